"""Every prox / dual-update kernel, bit for bit, through M = mu I.  GPU only.

The second half of the ADMM step -- z = prox(x + u), u += x - z, rhs = (z - u)/mu, ||x - z||, stop if < tol -- exists five times for single
handles (DESIGN.md 6.4 has the table): admm_small_iter_kernel (1), admm_batch_prox_kernel (2), admm_prox_kernel with its three top-r
selections (3), admm_fused_update2_kernel + admm_commit_kernel (4) and the prologue of admm_iter_mixed_kernel (5).  A handle built from a
zero Gram and a zero right-hand side with mu = 2^-k has H = I/mu, M = mu I and xb = 0, exactly, in every storage.  From an injected
state (z0, u0) one iteration forms x1 = M (z0 - u0)/mu = z0 - u0 and v = x1 + u0 = z0 -- exact for the inputs used here, which the test
CHECKS (a failed check fails, it does not skip) -- so everything that rounds happens inside the update, and tests/_prox_ref.py (held to
the CPU oracle and to the definitions by tests/test_prox_ref_host.py) restates it operation for operation: x, z, u after one and after
two iterations (x2 = z1 - u1 shows rhs1), ||x - z||, the iteration count and the converged flag of every signal slot must EQUAL the
model's.  ||x - z|| is compared with == where the model proves the sum exact in any order (_prox_ref.sum_is_exact) and is held to
(n + 2) 2^-53 relative otherwise.  The one-launch iteration rounds x to its quantum q: the test bounds q from above for every launch and
checks that the model's x is a multiple of it.

The default options stay on (mixed32 storage, x-update correction, mirrored tile order): the correction is first due after iteration 16
and the stale-nibble refresh multiplies zero nibbles.  Window batches (admm_window_update_kernel, and admm_fused_update_kernel behind
them) have no state entry and stay out of scope, as in tests/test_gpu_packed_inverse.py.
"""
import time

import numpy as np
import pytest

import _prox_ref as P
from _guards import precondition_not_met

pytestmark = pytest.mark.gpu

LPV_SHAPES = {130: (13, 5), 1000: (125, 4), 1900: (190, 5), 1920: (120, 8), 2112: (132, 8), 8320: (520, 8), 32784: (2049, 8)}   # n = 2 Nf Nv
COUNTS = {}           # route -> [elements compared, cut / tie / special elements met]
TIMES = {}            # handle -> seconds to build


def _np(n):
    return -(-n // 128) * 128


def _fusable(n, kind, gl):
    """fused_ok (csrc/admm.hip)."""
    return kind in (P.L1, P.L0) or (kind == P.GROUP and gl <= 128 and 128 % gl == 0 and n % gl == 0)


def route_of(n, ns, kind, gl, iteration):
    """The dispatch of launch_admm_iterations (csrc/admm.hip) restated: which copy of the update a handle runs."""
    if _np(n) < 2048:                                   # the full matrix (kSymmetricMinNp is a bound on the PADDED size: n = 2047 is not here)
        if kind == P.BALL:
            return 3
        small = iteration != "two" and (kind in (P.L1, P.L0) or (1 <= gl <= 256 and n % gl == 0))     # small_iter_applicable
        assert n <= 4096
        return 1 if small else 2
    if not _fusable(n, kind, gl):
        return 3
    return 5 if ns == 1 and iteration != "two" else 4


def _expected_info(route, n, ns, f32):
    if route == 1:
        return "admm_small_iter_kernel", True
    if _np(n) < 2048:
        return "symv_kernel", False
    if route == 5:
        return "admm_iter_mixed_kernel", True
    return ("symv_tile_mfma_ws_kernel" if ns > 1 else "symv_tile_f32_kernel" if f32 else "symv_tile_mixed_kernel"), False


def _zero_lpv(L, n, ns, f32):
    """An LPV handle from a zero record whose Gram is zeroed on the device (the pad block stays as the library made it)."""
    import torch
    Nf, Nv = LPV_SHAPES[n]
    N = 4096 if n > 30000 else 256
    rng = np.random.default_rng(n)
    X = np.sort(rng.random(N) * 10.0); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    dt = np.float32 if f32 else np.float64
    X, V, w = (a.astype(dt) for a in (X, V, w))
    p = L.Problem.lpv_multi(np.zeros((N, ns), dtype=dt, order="F"), X, V, w, Nv) if ns > 1 else L.Problem.lpv(np.zeros(N, dtype=dt), X, V, w, Nv)
    assert p.n == n and p.ns == ns and bool(p.f32) == f32
    Gd, _ = p.device_gram()
    Gd[:n, :n].zero_()
    torch.cuda.synchronize()
    p.gram_modified()
    return p


@pytest.fixture(scope="module")
def handles(L):
    cache = {}

    def get(n, ns=1, f32=False):
        key = (n, ns, f32)
        if key not in cache:
            t0 = time.perf_counter()
            if ns == 1 and not f32 and n < 30000:
                p = L.Problem.gram(np.zeros((n, n), order="F"), np.zeros(n))
            else:
                p = _zero_lpv(L, n, ns, f32)
            assert not np.any(p.get_rhs()), "a zero record must give b = 0"
            if n <= 2112:                                # the whole inverse is mu I, entry by entry (larger sizes: the x of every case says so)
                M = p.get_inverse(2.0 ** 4)
                assert np.array_equal(M, 2.0 ** -4 * np.eye(n)), "M = mu I must hold exactly"
            p.set_prox(L.NormL1(1.0))
            p.admm_init(None, μ=2.0 ** -4, tol=0.0)      # (the factorisation and the packing of the inverse belong to the build time)
            TIMES[key] = time.perf_counter() - t0
            cache[key] = p
        return cache[key]
    yield get
    for p in cache.values():
        p.close()
    for key, t in sorted(TIMES.items()):
        print(f"[prox-update build] n={key[0]} ns={key[1]} f32={key[2]}: {t:.2f} s")
    for route, (els, cuts) in sorted(COUNTS.items()):         # the totals DESIGN 6.4 quotes
        print(f"[prox-update total] route {route}: {els} elements compared, {cuts} cut / tie / special elements met")


def _prox_obj(L, kind, param, gl):
    if kind == P.L1:
        return L.NormL1(param)
    if kind == P.L0:
        return L.NormL0(param)
    if kind == P.BALL:
        return L.IndBallL0(int(param))
    return L.SlicedSeparableSum.frequency_groups(param, 1, gl)


def _first_diff(name, got, ref):
    bad = got != ref
    if np.isnan(got).any():
        return f"{name}: NaN at {np.flatnonzero(np.isnan(got))[:5]}"
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return f"{name}: {int(bad.sum())} of {bad.size} differ; first at {i} (block {i // 128}): device {got[i]!r}, model {ref[i]!r}"


def _quantum_upper(m, mu, upto):
    """An upper bound of the one-launch quantum of every launch up to iteration `upto` (csrc/admm_one_launch.hip: q = 2^(e - 62),
    R ((max|xb| + R max|rhs| + max|u|) / mu) 1.000001 < 2^e, R = mu, xb = 0), from the maxima over ALL earlier right-hand sides and duals."""
    mR = max(float(np.abs(h["rhs"]).max()) for h in m["pre"][:upto])
    mU = max(float(np.abs(h["u"]).max()) for h in m["pre"][:upto])
    B = mu * ((mu * mR + mU) / mu) * 1.000001
    _, e = np.frexp(max(B, 2.0 ** -900))
    return float(np.ldexp(1.0, int(e) - 62))


def run_case(L, p, route, kind, param, gl, mu, Z0, U0, iters_list=(1, 2), tol=0.0, iteration=None, marks=0, label=""):
    """One prox on one handle from the state (0, Z0, U0) (columns = signal slots): route as declared, then after each count of
    `iters_list` (one admm_run call each) x, z, u, ||x - z||, iterations and converged of every slot against the model."""
    n, ns, f32 = p.n, p.ns, bool(p.f32)
    Z0 = np.asfortranarray(Z0.reshape(n, ns)); U0 = np.asfortranarray(U0.reshape(n, ns))
    assert route_of(n, ns, kind, gl, iteration) == route, (label, "the dispatch rule sends this case to route", route_of(n, ns, kind, gl, iteration))
    p.set_option("iteration", iteration)
    p.set_prox(_prox_obj(L, kind, param, gl))
    p.admm_init(None, μ=mu, tol=tol)
    info = p.matvec_info()
    assert (info["kernel"], bool(info.get("one_launch_iteration", False))) == _expected_info(route, n, ns, f32), (label, route, info)
    dt = np.float32 if f32 else np.float64
    if f32 and not (np.array_equal(Z0.astype(dt).astype(np.float64), Z0) and np.array_equal(U0.astype(dt).astype(np.float64), U0)):
        precondition_not_met(f"{label}: the state of an _f32 handle must be representable in float")
    zero = np.zeros((n, ns), dtype=dt, order="F")
    sq = (lambda a: a if ns > 1 else a[:, 0])
    for k in iters_list:
        p.admm_set_state(sq(zero), sq(Z0.astype(dt)), sq(U0.astype(dt)), iters=0)
        p.admm_run(k)
        got = [a.reshape(n, ns, order="F") for a in p.admm_get(f64=True)]
        for q in range(ns):
            m = P.iterate(Z0[:, q], U0[:, q], mu, kind, param, gl, tol=tol, iters=k)
            h0 = m["hist"][0]
            # the exactness argument, checked: x1 = z0 - u0 and v = z0 without rounding, no NaN / inf anywhere in the model
            ld = np.longdouble
            if not (np.array_equal(h0["x"].astype(ld), Z0[:, q].astype(ld) - U0[:, q].astype(ld)) and np.array_equal(h0["v"], Z0[:, q])):
                precondition_not_met(f"{label}: x1 = z0 - u0 or v = z0 rounds for this state")
            if not all(np.isfinite(h[a]).all() for h in m["hist"] for a in ("x", "z", "u", "rhs")):
                precondition_not_met(f"{label}: the model meets a non-finite value")
            if route == 5:
                m["pre"] = [dict(rhs=(Z0[:, q] - U0[:, q]) / mu, u=U0[:, q])] + m["hist"]
                for j, h in enumerate(m["hist"]):
                    qu = _quantum_upper(m, mu, j + 1)
                    if np.any(np.fmod(h["x"], qu) != 0):
                        precondition_not_met(f"{label}: x{j + 1} of the model is no multiple of the one-launch quantum (<= {qu!r})")
            msgs = [_first_diff(nm, g[:, q], m[nm]) for nm, g in zip("xzu", got)]
            assert not any(msgs), (label, f"route {route} n={n} slot {q} after admm_run({k})", [s for s in msgs if s])
            it, nxz, conv = p.admm_status(q)
            assert (it, conv) == (m["iters"], m["converged"]), (label, route, n, q, k, (it, conv), (m["iters"], m["converged"]))
            if m["nxz_exact"]:
                assert nxz == m["nxz"], (label, route, n, q, k, nxz, m["nxz"])
            else:
                assert abs(nxz - m["nxz"]) <= P.nxz_bound(n) * m["nxz"], (label, route, n, q, k, nxz, m["nxz"])
            c = COUNTS.setdefault(route, [0, 0])
            c[0] += 3 * n
            c[1] += marks
    return info


# ---- the handles of every route: (route, n, ns, f32) ---------------------------------------------------------------------------
# (the full-matrix routes end at np = 1920: kSymmetricMinNp = 2048 bounds the PADDED size, so n = 2047 (np = 2048) is a packed handle and
# runs routes 4 / 5 here; LPV sizes are even, so the several-signal handle next to the threshold is n = 1920; n = 1792 = 7 * 256 takes
# gl = 256, the largest group of route 1)
R1 = [(1, 130, 1), (1, 1000, 1), (1, 1792, 1), (1, 1920, 1), (1, 130, 3), (1, 1000, 3), (1, 1920, 3)]
R2 = [(2, 1000, 1), (2, 1900, 1), (2, 1000, 3), (2, 1900, 3)]
R3 = [(3, 1900, 1), (3, 2112, 1), (3, 8320, 1), (3, 2112, 3)]
R4 = [(4, 2047, 1), (4, 2112, 1), (4, 8320, 1), (4, 2112, 3), (4, 8320, 3)]
R5 = [(5, 2047, 1), (5, 2112, 1), (5, 8320, 1), (5, 2112, 1, True)]
ELEMENTWISE = R1 + R2 + R4 + R5                     # (L1 / L0 are fusable everywhere: route 3 never sees them)


def _id(h):
    return f"route{h[0]}-n{h[1]}-ns{h[2]}" + ("-f32" if len(h) > 3 and h[3] else "")


def _get(handles, h):
    return handles(h[1], h[2], len(h) > 3 and h[3]), (len(h) > 3 and h[3])


def _iteration(route):
    return "two" if route in (2, 4) else None


def _slots(ns, fn):
    """An n x ns state, every slot its own vector: fn(q)."""
    return np.stack([fn(q) for q in range(ns)], axis=1)


# ---- 1. dense dyadic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [P.L1, P.L0], ids=["l1", "l0"])
@pytest.mark.parametrize("h", ELEMENTWISE, ids=_id)
def test_dense_dyadic_states_elementwise(L, handles, h, kind):
    p, f32 = _get(handles, h)
    rng = np.random.default_rng(h[1] + 10 * h[2] + kind)
    bits = 20 if f32 else 40
    c = P.L1_CUT if kind == P.L1 else P.L0_CUT
    Z0 = _slots(p.ns, lambda q: P.dyadic(p.n, rng, bits))
    for name, U0 in (("u0=0", np.zeros_like(Z0)), ("u0!=0", _slots(p.ns, lambda q: P.dyadic(p.n, rng, bits)))):
        run_case(L, p, h[0], kind, c["param"], 0, c["mu"], Z0, U0, iteration=_iteration(h[0]), label=f"dense dyadic {name}")


# ---- 2. / 3. the cuts of L1 and L0 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [P.L1, P.L0], ids=["l1", "l0"])
@pytest.mark.parametrize("h", ELEMENTWISE, ids=_id)
def test_cuts_of_l1_and_l0(L, handles, h, kind):
    """v == +-g, its two neighbours and 0 at index 0, n - 1 and both sides of every multiple of 128: `<=` / `>=` of the soft threshold,
    the strict `>` of the hard one (|v| == 0.5 gives 0, its upper neighbour is kept)."""
    p, f32 = _get(handles, h)
    rng = np.random.default_rng(h[1] + kind)
    c, cut = (P.L1_CUT, 0.25) if kind == P.L1 else (P.L0_CUT, 0.5)
    vs = [P.cuts(p.n, rng, cut, shift=2 * q, f32=f32) for q in range(p.ns)]
    Z0 = np.stack([v for v, _ in vs], axis=1)
    if kind == P.L0:
        z = P.prox(kind, Z0[:, 0], c["param"], c["mu"])
        at, up = np.abs(Z0[:, 0]) == cut, np.abs(Z0[:, 0]) == P.cut_values(cut, f32)[2]
        assert at.sum() >= 2 and not z[at].any() and up.sum() >= 2 and z[up].all()
    run_case(L, p, h[0], kind, c["param"], 0, c["mu"], Z0, np.zeros_like(Z0), iteration=_iteration(h[0]), marks=len(vs[0][1]), label="cuts")


# ---- 4. group prox ---------------------------------------------------------------------------------------------------------------------
def _group_cases():
    out = []
    for h in R1:
        for gl in (1, 2, 3, 5, 13, 64, 128, 200, 250, 256):
            if h[1] % gl == 0 and gl <= 256:
                out.append((h, gl, None))
    for h in R2:
        out += [(h, gl, "two") for gl in (3, 200, 256, 300)]
        out += [(h, gl, None) for gl in (256, 300) if not (gl <= 256 and h[1] % gl == 0)]      # not applicable to route 1: route 2 by default too
    for h in R3[1:]:
        gls = [3, 200] + ([8192] if h[1] == 8320 else [128])                                   # (128 at n = 2112: n % gl = 64, a tail)
        out += [(h, gl, None) for gl in gls if not _fusable(h[1], P.GROUP, gl)]
    for h in R4 + R5:
        out += [(h, gl, _iteration(h[0])) for gl in (1, 2, 64, 128) if _fusable(h[1], P.GROUP, gl)]
    return out


@pytest.mark.parametrize("h,gl,iteration", _group_cases(), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_group_prox(L, handles, h, gl, iteration):
    """Norm exactly lambda mu (z = 0), the next s2 above it, an all-zero group (no NaN), a one-hot group, the last group, groups on both
    sides of every multiple of 128, among dense groups; with a tail (n % gl != 0) the tail starts from a non-zero z0 and must come back
    unchanged while u moves."""
    p, f32 = _get(handles, h)
    n, route = p.n, h[0]
    rng = np.random.default_rng(n + gl)
    bits = 20 if f32 else 40
    vs = [P.group_input(n, gl, rng, bits=bits) for _ in range(p.ns)]
    Z0 = np.stack([v for v, _ in vs], axis=1)
    tail = n - (n // gl) * gl
    if tail:
        assert np.all(Z0[n - tail:] != 0)
    marks = vs[0][1] * gl + tail
    U0 = _slots(p.ns, lambda q: P.dyadic(n, rng, bits))
    U0 = np.where(np.fmod(Z0, 2.0 ** -bits) == 0, U0, 0.0)        # (x1 = z0 - u0 must not round: u0 = 0 where z0 is a neighbour of a cut)
    kw = dict(iteration=iteration, marks=marks)
    run_case(L, p, route, P.GROUP, P.GROUP_LAM, gl, P.GROUP_MU, Z0, np.zeros_like(Z0), label=f"group gl={gl} u0=0", **kw)
    run_case(L, p, route, P.GROUP, P.GROUP_LAM, gl, P.GROUP_MU, Z0, U0, label=f"group gl={gl} u0!=0", **kw)


def test_group_len_8193_is_refused_and_8192_is_not(L, handles):
    p = handles(8320)
    with pytest.raises(NotImplementedError):
        p.set_prox(L.SlicedSeparableSum.frequency_groups(1.0, 1, 8193))
    p.set_prox(L.SlicedSeparableSum.frequency_groups(1.0, 1, 8192))       # (run by test_group_prox: one group per pass and a tail of 128)


# ---- 5. IndBallL0 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", R3 + [(3, 32784, 1)], ids=_id)
def test_ball_selection(L, handles, h):
    """Every selection level of admm_prox_kernel: the 11-bit histogram with up to 1023 candidates, the byte-wise select on float keys
    behind it, the 64-bit select (with and without ties at the threshold, the carried count of equal keys across 8192-element passes),
    the scratch copy of v (n > 8192) and the direct entry (n > 32768)."""
    p, _ = _get(handles, h)
    n, big = p.n, p.n > 32768
    rngs = [np.random.default_rng(n + 100 * q) for q in range(p.ns)]
    per_slot = [P.ball_inputs(n, r, big=big) for r in rngs]
    for ci, (label, _, rs, cnt) in enumerate(per_slot[0]):
        Z0 = np.stack([c[ci][1] for c in per_slot], axis=1)
        for r in rs:
            for q in range(p.ns):
                assert int(P.ball_keep(Z0[:, q], r).sum()) == min(r, n)
            run_case(L, p, 3, P.BALL, r, 0, 2.0 ** -4, Z0, np.zeros_like(Z0), marks=cnt, label=f"ball {label} r={r}")
    Z0 = _slots(p.ns, lambda q: P.dyadic(n, rngs[q], 40))                  # ... and a state with u0 != 0
    run_case(L, p, 3, P.BALL, 32, 0, 2.0 ** -4, Z0, _slots(p.ns, lambda q: P.dyadic(n, rngs[q], 40)), label="ball dense dyadic u0!=0")


# ---- 6. the stopping test ------------------------------------------------------------------------------------------------------------
def _stop_cases():
    out = []
    for h in R1 + R2 + R4 + R5:
        out += [(h, P.L1, 0), (h, P.L0, 0)]
        gl = 64 if h[1] % 64 == 0 else (5 if h[1] % 5 == 0 else 23)
        if h[0] == 2 or route_of(h[1], h[2], P.GROUP, gl, _iteration(h[0])) == h[0]:
            out.append((h, P.GROUP, 300 if h[0] == 2 else gl))
    for h in R3:
        out.append((h, P.BALL, 0))
        if h[1] >= 2048:
            out.append((h, P.GROUP, 200))
    return out


@pytest.mark.parametrize("h,kind,gl", _stop_cases(), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_stopping_test_is_strict_and_reported_in_its_iteration(L, handles, h, kind, gl):
    """Slot 0: d = x1 - z1 = (3, 4, 0, ...) 2^-5 in two different row blocks, ||x - z|| = 5 * 2^-5 exactly.  tol = that norm: iteration 1
    must not stop (strict <, src/lasso.jl:164); tol = the next double: it stops there, and x, z, u stay those of iteration 1 over the two
    further iterations of admm_run(3) while the other slots (dense, far from tol) move.  The routes that defer the test by a launch must
    report the model's iteration."""
    p, f32 = _get(handles, h)
    n, route = p.n, h[0]
    rng = np.random.default_rng(n + kind)
    K = 4
    last = ((n // gl) * gl if gl else n) - 2
    z0 = np.zeros(n); z0[1], z0[last] = 3 * 2.0 ** -5, -4 * 2.0 ** -5
    param, mu = {P.L1: (4.0, 2.0 ** -4), P.L0: (1.0, 2.0 ** -3), P.GROUP: (P.GROUP_LAM, P.GROUP_MU), P.BALL: (K, 2.0 ** -4)}[kind]
    if kind == P.BALL:
        z0[[7, 300, n // 2, n - 5]] = [2.0, -3.0, 4.0, -5.0]
    Z0 = _slots(p.ns, lambda q: z0 if q == 0 else P.dyadic(n, rng, 9))
    nxz = 5 * 2.0 ** -5
    m = P.iterate(z0, np.zeros(n), mu, kind, param, gl, tol=0.0, iters=1)
    if not (m["nxz_exact"] and m["nxz"] == nxz):
        precondition_not_met(f"the state of slot 0 must give ||x - z|| = 5 * 2^-5 exactly, the model says {m['nxz']!r}")
    for tol, stops in ((nxz, False), (float(np.nextafter(nxz, np.inf)), True)):
        m = P.iterate(z0, np.zeros(n), mu, kind, param, gl, tol=tol, iters=3)
        assert (m["iters"] == 1 and m["converged"]) == stops
        run_case(L, p, route, kind, param, gl, mu, Z0, np.zeros_like(Z0), iters_list=(1, 3), tol=tol, iteration=_iteration(route), marks=2,
                 label=f"stopping tol={'nxz' if not stops else 'next(nxz)'}")


# ---- 7. wide range (routes 2, 3, 4; u0 = 0) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [P.L1, P.L0], ids=["l1", "l0"])
@pytest.mark.parametrize("h", R2 + R4, ids=_id)
def test_wide_range_elementwise(L, handles, h, kind):
    p, _ = _get(handles, h)
    rng = np.random.default_rng(h[1] + kind)
    c = P.L1_CUT if kind == P.L1 else P.L0_CUT
    Z0 = _slots(p.ns, lambda q: P.wide_values(p.n, rng))
    run_case(L, p, h[0], kind, c["param"], 0, c["mu"], Z0, np.zeros_like(Z0), iteration="two", label="wide range 2^-1060 .. 2^990")


@pytest.mark.parametrize("h", R3, ids=_id)
def test_wide_range_ball(L, handles, h):
    """Float keys +inf (|v| > FLT_MAX) and 0 (|v| < 2^-149) with the cut between them: only the doubles tell the candidates apart."""
    p, _ = _get(handles, h)
    rngs = [np.random.default_rng(h[1] + 7 * q) for q in range(p.ns)]
    per_slot = [P.wide_ball(p.n, r) for r in rngs]
    for ci, (label, _, rs, cnt) in enumerate(per_slot[0]):
        Z0 = np.stack([c[ci][1] for c in per_slot], axis=1)
        for r in rs:
            run_case(L, p, 3, P.BALL, r, 0, 2.0 ** -4, Z0, np.zeros_like(Z0), marks=cnt, label=f"ball {label} r={r}")


@pytest.mark.parametrize("h,gl,iteration", [(h, 300, "two") for h in R2] + [(h, 200, None) for h in R3[1:]] + [(h, 64, "two") for h in R4 if h[1] % 64 == 0],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_wide_range_group(L, handles, h, gl, iteration):
    """A group whose s2 overflows (scale 1, z = v) and one whose s2 underflows to 0 (z = 0)."""
    p, _ = _get(handles, h)
    rng = np.random.default_rng(h[1] + gl)
    Z0 = _slots(p.ns, lambda q: P.wide_group(p.n, gl, rng))
    z = P.prox(P.GROUP, Z0[:, 0], P.GROUP_LAM, P.GROUP_MU, gl)
    ng = p.n // gl
    assert np.array_equal(z[gl:2 * gl], Z0[gl:2 * gl, 0]) and not z[(ng - 1) * gl:ng * gl].any()
    run_case(L, p, h[0], P.GROUP, P.GROUP_LAM, gl, P.GROUP_MU, Z0, np.zeros_like(Z0), iteration=iteration, marks=2 * gl, label=f"wide group gl={gl}")
