"""Per-signal prox parameters on one shared inverse (a regularisation path).  GPU only.

1. Every update kernel a handle with several signals can reach, bit for bit, with a DIFFERENT parameter in every slot: the method of
   tests/test_gpu_prox_update.py -- a zero-Gram LPV multi handle, mu = 2^-k, M = mu I exactly, state injected with admm_set_state, and
   tests/_prox_ref.py as the model, iterated per signal with that signal's parameter.
2. Uniform per-signal parameters give the bits of the scalar.
3. A column of a path is that penalty's own solve, bit for bit, across the correction at iteration 16.
4. lpvs_problem_create_path from every constructor: the Gram and every right-hand side are the source's bits, column q is the
   single-signal estimator's result with lambda_q, the source may be destroyed first.
5. lambda_max: 1.01 lambda_max gives z = 0 exactly, 0.9 lambda_max does not, both converge.
6. The error returns, each leaving the handle usable.

Bounds: == everywhere except where the issue that introduced this file allows rel <= 1e-11 (the default one-launch route of test 4; the
figure tests/test_gpu_xupdate_correction.py uses for multi against single), and ||x - z|| as tests/test_gpu_prox_update.py compares it
(== where _prox_ref.sum_is_exact, (n + 2) 2^-53 relative otherwise).
"""
import ctypes as C

import numpy as np
import pytest

import _prox_ref as P
from _guards import precondition_not_met

pytestmark = pytest.mark.gpu

LPV_SHAPES = {130: (13, 5), 2112: (132, 8)}                      # n = 2 Nf Nv (entries of test_gpu_prox_update.LPV_SHAPES)
SMALL, BATCH, WS = "admm_small_iter_kernel", "symv_kernel", "symv_tile_mfma_ws_kernel"


def _zero_lpv(L, n, ns):
    """An LPV multi handle from a zero record whose Gram is zeroed on the device: M = mu I, b = 0."""
    import torch
    Nf, Nv = LPV_SHAPES[n]
    N = 256
    rng = np.random.default_rng(n)
    X = np.sort(rng.random(N) * 10.0); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    p = L.Problem.lpv_multi(np.zeros((N, ns), order="F"), X, V, w, Nv)
    assert p.n == n and p.ns == ns and not p.f32
    Gd, _ = p.device_gram()
    Gd[:n, :n].zero_()
    torch.cuda.synchronize()
    p.gram_modified()
    return p


@pytest.fixture(scope="module")
def handles(L):
    cache = {}

    def get(n, ns):
        if (n, ns) not in cache:
            p = _zero_lpv(L, n, ns)
            assert not np.any(p.get_rhs()), "a zero record must give b = 0"
            assert np.array_equal(p.get_inverse(2.0 ** 4), 2.0 ** -4 * np.eye(n)), "M = mu I must hold exactly"
            cache[(n, ns)] = p
        return cache[(n, ns)]
    yield get
    for p in cache.values():
        p.close()


def _first_diff(name, got, ref):
    bad = got != ref
    if np.isnan(got).any():
        return f"{name}: NaN at {np.flatnonzero(np.isnan(got))[:5]}"
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return f"{name}: {int(bad.sum())} of {bad.size} differ; first at {i} (block {i // 128}): device {got[i]!r}, model {ref[i]!r}"


def run_case(p, kernel, kind, params, gl, mu, Z0, U0, iters_list=(1, 2), tol=0.0, iteration=None, label=""):
    """Slot q runs prox `kind` with params[q] from the state (0, Z0[:, q], U0[:, q]): the kernel as declared, then after each count of
    `iters_list` x, z, u, ||x - z||, iterations and converged of every slot against the model with THAT slot's parameter."""
    n, ns = p.n, p.ns
    params = [float(v) for v in params]
    assert len(params) == ns and Z0.shape == U0.shape == (n, ns)
    Z0, U0 = np.asfortranarray(Z0), np.asfortranarray(U0)
    p.set_option("iteration", iteration)
    p.set_prox_params(kind, params, gl)
    assert p.get_prox_params().tolist() == params
    p.admm_init(None, μ=mu, tol=tol)
    info = p.matvec_info()
    assert (info["kernel"], bool(info.get("one_launch_iteration", False))) == (kernel, kernel == SMALL), (label, info)
    zero = np.zeros((n, ns), order="F")
    models = {}
    for k in iters_list:
        p.admm_set_state(zero, Z0, U0, iters=0)
        p.admm_run(k)
        got = [a.reshape(n, ns, order="F") for a in p.admm_get(f64=True)]
        for q in range(ns):
            m = models[(k, q)] = P.iterate(Z0[:, q], U0[:, q], mu, kind, params[q], gl, tol=tol, iters=k)
            h0 = m["hist"][0]
            ld = np.longdouble   # the exactness argument, checked: x1 = z0 - u0 and v = z0 without rounding, nothing non-finite
            if not (np.array_equal(h0["x"].astype(ld), Z0[:, q].astype(ld) - U0[:, q].astype(ld)) and np.array_equal(h0["v"], Z0[:, q])):
                precondition_not_met(f"{label}: x1 = z0 - u0 or v = z0 rounds for the state of slot {q}")
            if not all(np.isfinite(h[a]).all() for h in m["hist"] for a in ("x", "z", "u", "rhs")):
                precondition_not_met(f"{label}: the model meets a non-finite value")
            msgs = [_first_diff(nm, g[:, q], m[nm]) for nm, g in zip("xzu", got)]
            assert not any(msgs), (label, f"{kernel} n={n} slot {q} param {params[q]!r} after admm_run({k})", [s for s in msgs if s])
            it, nxz, conv = p.admm_status(q)
            assert (it, conv) == (m["iters"], m["converged"]), (label, kernel, n, q, k, (it, conv), (m["iters"], m["converged"]))
            if m["nxz_exact"]:
                assert nxz == m["nxz"], (label, kernel, n, q, k, nxz, m["nxz"])
            else:
                assert abs(nxz - m["nxz"]) <= P.nxz_bound(n) * m["nxz"], (label, kernel, n, q, k, nxz, m["nxz"])
    return models


def _slots(ns, fn):
    return np.stack([fn(q) for q in range(ns)], axis=1)


# the multipliers of a slot's parameter: slot 0 holds the cut parameter of _prox_ref itself, its neighbours are scaled by powers of two
# (of four: sqrt(2 mu lambda) of NormL0 stays exact), one slot holds 0 (L1: the identity)
SCALE = {8: [1.0, 4.0, 0.25, 0.0, 16.0, 2.0 ** -4, 64.0, 2.0 ** -6], 3: [1.0, 4.0, 0.0]}

# (kernel, n, iteration): the update behind each -- admm_small_iter_kernel's own, admm_batch_prox_kernel, admm_fused_update2_kernel
ELEMENTWISE = [(SMALL, 130, None), (BATCH, 130, "two"), (WS, 2112, None)]
GROUPS = [(SMALL, 130, None, 13), (BATCH, 130, "two", 13), (WS, 2112, None, 8),
          (WS, 2112, None, 3)]                                    # gl = 3: 128 % 3 != 0, not fusable -> admm_prox_kernel's group branch


def _id(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ---- 1a. L1 / L0: the cuts of slot 0 in every slot, then every slot's own cuts ------------------------------------------------------
@pytest.mark.parametrize("ns", [8, 3])
@pytest.mark.parametrize("kind", [P.L1, P.L0], ids=["l1", "l0"])
@pytest.mark.parametrize("h", ELEMENTWISE, ids=_id)
def test_elementwise_parameter_per_slot(L, handles, h, kind, ns):
    kernel, n, iteration = h
    p = handles(n, ns)
    rng = np.random.default_rng(n + 10 * ns + kind)
    c, cut = (P.L1_CUT, 0.25) if kind == P.L1 else (P.L0_CUT, 0.5)
    params = [c["param"] * s for s in SCALE[ns]]
    cut_of = (lambda lam: c["mu"] * lam) if kind == P.L1 else (lambda lam: float(np.sqrt(2.0 * c["mu"] * lam)))
    # the same input in every slot: v == +-cut(slot 0), its neighbours and a dense 2^-12 grid in [0, 2) -- cut in one slot, kept in the next
    v, pos = P.cuts(n, rng, cut)
    Z0 = _slots(ns, lambda q: v)
    m = run_case(p, kernel, kind, params, 0, c["mu"], Z0, np.zeros_like(Z0), iteration=iteration, label="shared cuts")
    z1 = np.stack([m[(1, q)]["z"] for q in range(ns)], axis=1)
    at = np.abs(v) == cut
    assert at.sum() >= 2 and not z1[at, 0].any(), "slot 0 cuts its own cut value"
    assert z1[at, 2].all() and not z1[at, 1].any(), "the slot with a quarter of the parameter keeps it, the slot with four times cuts it"
    if kind == P.L1:
        assert np.array_equal(z1[:, SCALE[ns].index(0.0)], v), "parameter 0 is the identity"
    assert len({z1[:, q].tobytes() for q in range(ns)}) >= ns - 1, "the slots must differ"
    # every slot its own cut values (a slot whose parameter is 0: around slot 0's cut), and a dual that is not zero
    Z0 = _slots(ns, lambda q: P.cuts(n, rng, cut_of(params[q]) or cut, shift=2 * q)[0])
    run_case(p, kernel, kind, params, 0, c["mu"], Z0, np.zeros_like(Z0), iteration=iteration, label="own cuts")
    Z0 = _slots(ns, lambda q: P.dyadic(n, rng, 40))
    run_case(p, kernel, kind, params, 0, c["mu"], Z0, _slots(ns, lambda q: P.dyadic(n, rng, 40)), iteration=iteration, label="dense dyadic u0!=0")


# ---- 1b. the group prox -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [8, 3])
@pytest.mark.parametrize("h", GROUPS, ids=_id)
def test_group_parameter_per_slot(L, handles, h, ns):
    kernel, n, iteration, gl = h
    p = handles(n, ns)
    rng = np.random.default_rng(n + gl + ns)
    params = [P.GROUP_LAM * s for s in SCALE[ns]]
    v, _ = P.group_input(n, gl, rng)              # groups of norm exactly GROUP_LAM GROUP_MU, the next s2 above, all-zero, one-hot
    Z0 = _slots(ns, lambda q: v)
    m = run_case(p, kernel, P.GROUP, params, gl, P.GROUP_MU, Z0, np.zeros_like(Z0), iteration=iteration, label=f"group gl={gl} shared")
    z1 = np.stack([m[(1, q)]["z"] for q in range(ns)], axis=1)
    s2 = P.group_s2(v, gl)
    exact = np.flatnonzero(s2 == (P.GROUP_LAM * P.GROUP_MU) ** 2)
    assert exact.size >= 1
    g = int(exact[0])
    assert not z1[g * gl:(g + 1) * gl, 0].any() and not z1[g * gl:(g + 1) * gl, 1].any() and z1[g * gl:(g + 1) * gl, 2].any(), \
        "a group of norm lambda mu: zero in slot 0 and under four times the penalty, kept under a quarter of it"
    assert np.array_equal(z1[:(n // gl) * gl, SCALE[ns].index(0.0)], v[:(n // gl) * gl]), "penalty 0: every whole group is kept as it is"
    Z0 = _slots(ns, lambda q: P.group_input(n, gl, rng)[0])
    U0 = _slots(ns, lambda q: P.dyadic(n, rng, 40))
    U0 = np.where(np.fmod(Z0, 2.0 ** -40) == 0, U0, 0.0)          # (x1 = z0 - u0 must not round: u0 = 0 where z0 is a neighbour of a cut)
    run_case(p, kernel, P.GROUP, params, gl, P.GROUP_MU, Z0, U0, iteration=iteration, label=f"group gl={gl} own u0!=0")


def _distinct(n, rng):
    """n distinct |v| (a permutation of 1 .. n times 2^-12), random signs."""
    return (rng.permutation(n) + 1.0) * 2.0 ** -12 * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _ties(n, rng):
    """(v, K, T): K distinct values above T exact ties of |v| = 3 with mixed signs, spread over the index range (different 1024-thread
    chunks at n = 2112), above a dense 2^-30 grid below 0.25 -- the layout of _prox_ref.ball_inputs' "ties", for any n >= 130."""
    K = 5
    v = P.dyadic(n, rng, bits=30, hi=0.25)
    top = rng.choice(n, K, replace=False)
    v[top] = (4.0 + np.arange(K)) * np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    taken, idx = set(int(i) for i in top), []
    for i in [5, n // 4, n // 3, n // 2, (2 * n) // 3, n - 3] + ([1030, 1100] if n > 1100 else []):
        while i in taken or i in idx:
            i += 1
        idx.append(i)
    idx = sorted(idx)
    v[idx] = 3.0 * np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0)
    return v, K, len(idx)


# ---- 1c. IndBallL0: r_q = (long long) params[q] -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [8, 3])
@pytest.mark.parametrize("h", [(BATCH, 130), (WS, 2112)], ids=_id)
def test_ball_radius_per_slot(L, handles, h, ns):
    """admm_prox_kernel with a distinct r in every slot, r = 0 (z = 0) and r >= n (z = v) among them: distinct |v| per slot, then one
    vector with exact ties in every slot so that the cut falls before, inside and behind the tied set."""
    kernel, n = h
    p = handles(n, ns)
    rngs = [np.random.default_rng(n + 100 * q) for q in range(ns)]
    rs = [0, 1, 2, 32, n // 2, n - 1, n, n + 5] if ns == 8 else [0, 32, n + 5]
    Z0 = _slots(ns, lambda q: _distinct(n, rngs[q]))
    for q in range(ns):
        assert int(P.ball_keep(Z0[:, q], rs[q]).sum()) == min(rs[q], n)
    m = run_case(p, kernel, P.BALL, rs, 0, 2.0 ** -4, Z0, np.zeros_like(Z0), label="ball distinct")
    assert not m[(1, 0)]["z"].any() and np.array_equal(m[(1, ns - 1)]["z"], Z0[:, ns - 1])
    v, K, T = _ties(n, rngs[0])
    rs = [K + T // 2, 0, K + 1, K + T - 1, n, K, K + T, 3] if ns == 8 else [K + T // 2, 0, n]
    Z0 = _slots(ns, lambda q: v)
    for q in range(ns):
        assert int(P.ball_keep(v, rs[q]).sum()) == min(rs[q], n)
    run_case(p, kernel, P.BALL, rs, 0, 2.0 ** -4, Z0, np.zeros_like(Z0), label="ball ties")
    Z0 = _slots(ns, lambda q: P.dyadic(n, rngs[q], 40))
    run_case(p, kernel, P.BALL, rs, 0, 2.0 ** -4, Z0, _slots(ns, lambda q: P.dyadic(n, rngs[q], 40)), label="ball dense dyadic u0!=0")


# ---- 1d. one slot stops at iteration 1, the others go on ----------------------------------------------------------------------------------
def _stop_cases():
    out = []
    for kernel, n, iteration in ELEMENTWISE:
        out += [(kernel, n, iteration, P.L1, 0), (kernel, n, iteration, P.L0, 0)]
    out += [(k, n, it, P.GROUP, gl) for k, n, it, gl in GROUPS]
    out += [(BATCH, 130, None, P.BALL, 0), (WS, 2112, None, P.BALL, 0)]
    return out


@pytest.mark.parametrize("ns", [8, 3])
@pytest.mark.parametrize("h", _stop_cases(), ids=_id)
def test_one_slot_stops_the_others_go_on(L, handles, h, ns):
    """Slot 0: d = x1 - z1 = (3, 4, 0, ...) 2^-5, ||x - z|| = 5 * 2^-5 exactly, tol = the next double: it stops at iteration 1 and its
    x, z, u stay those of iteration 1 over the two further iterations of admm_run(3), while the dense slots (far from tol, each under its
    own parameter) go on: through M = mu I they reach x = z in their second or third iteration, and the model says in which.  (A slot
    whose prox is the identity -- parameter 0, r >= n -- has x = z at once and stops with slot 0.)"""
    kernel, n, iteration, kind, gl = h
    p = handles(n, ns)
    rng = np.random.default_rng(n + kind + ns)
    last = ((n // gl) * gl if gl else n) - 2
    z0 = np.zeros(n); z0[1], z0[last] = 3 * 2.0 ** -5, -4 * 2.0 ** -5
    base, mu = {P.L1: (4.0, 2.0 ** -4), P.L0: (1.0, 2.0 ** -3), P.GROUP: (P.GROUP_LAM, P.GROUP_MU), P.BALL: (4, 2.0 ** -4)}[kind]
    if kind == P.BALL:
        z0[[7, n // 3, n // 2, n - 5]] = [2.0, -3.0, 4.0, -5.0]
        params = [4, 0, 1, 32, n // 2, n - 1, n, 7] if ns == 8 else [4, 32, n]
    else:
        params = [base * s for s in SCALE[ns]]
    Z0 = _slots(ns, lambda q: z0 if q == 0 else P.dyadic(n, rng, 9))
    nxz = 5 * 2.0 ** -5
    m0 = P.iterate(z0, np.zeros(n), mu, kind, params[0], gl, tol=0.0, iters=1)
    if not (m0["nxz_exact"] and m0["nxz"] == nxz):
        precondition_not_met(f"the state of slot 0 must give ||x - z|| = 5 * 2^-5 exactly, the model says {m0['nxz']!r}")
    tol = float(np.nextafter(nxz, np.inf))
    m = run_case(p, kernel, kind, params, gl, mu, Z0, np.zeros_like(Z0), iters_list=(1, 3), tol=tol, iteration=iteration, label="one slot stops")
    assert m[(3, 0)]["iters"] == 1 and m[(3, 0)]["converged"], "slot 0 must stop at iteration 1"
    moving = [q for q in range(1, ns) if m[(3, q)]["iters"] >= 2]
    assert len(moving) >= 1, "at least one slot must go on past iteration 1"
    assert any(not np.array_equal(m[(3, q)]["u"], m[(1, q)]["u"]) for q in moving), "the slots that go on must move"


# ---- 2. / 3. a real problem at n = 2112 -----------------------------------------------------------------------------------------------------
def _lpv_record(seed=7, N=4096, Nf=132, Nv=8, ns=4):
    rng = np.random.default_rng(seed)
    X = np.sort(10 * rng.random(N)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 0.2
    Y = np.stack([(2 + q) * V ** 2 * np.cos(w[5 + 3 * q] * X) + 3 * np.exp(-10 * (V - 0.5) ** 2) * np.cos(w[40 + q] * X + 0.1 * q)
                  + 0.1 * rng.standard_normal(N) for q in range(ns)], axis=1)
    return np.asfortranarray(Y), X, V, w, Nv


def _run(p, proxg, iters, tol=0.0):
    p.set_prox(proxg)
    p.admm_init(None, μ=0.05, tol=tol)
    p.admm_run(iters)
    return [a.copy() for a in p.admm_get(f64=True)], [p.admm_status(q) for q in range(p.ns)]


def _same(a, b, what):
    for nm, u, v in zip("xzu", a[0], b[0]):
        assert np.array_equal(u, v), (what, nm, int((u != v).sum()), float(np.abs(u - v).max()))
    assert a[1] == b[1], (what, a[1], b[1])


@pytest.fixture(scope="module")
def lpv2112(L):
    Y, X, V, w, Nv = _lpv_record()
    with L.Problem.lpv_multi(Y, X, V, w, Nv) as p, L.Problem.lpv_multi(np.asfortranarray(np.tile(Y[:, :1], (1, 4))), X, V, w, Nv) as pt:
        assert p.n == pt.n == 2112 and p.ns == pt.ns == 4
        yield p, pt, len(w), Nv


def test_uniform_parameters_are_the_scalar(L, lpv2112):
    p, _, Nf, Nv = lpv2112
    lam = 0.2 * float(np.min(L.lambda_max(p, L.SlicedSeparableSum, group_len=2 * Nv)))
    g = L.SlicedSeparableSum.frequency_groups(lam, Nf, 2 * Nv)
    scalar = _run(p, g, 40)
    assert p.matvec_info()["kernel"] == WS and p.get_prox_params().tolist() == [lam] * 4
    assert all(np.any(a) for a in scalar[0]) and all(s[0] == 40 for s in scalar[1])
    _same(_run(p, [g] * 4, 40), scalar, "set_prox([g] * 4) against set_prox(g)")
    other = _run(p, [L.SlicedSeparableSum.frequency_groups(lam * (q + 1), Nf, 2 * Nv) for q in range(4)], 40)
    assert not np.array_equal(other[0][1][:, 3], scalar[0][1][:, 3]), "a different penalty in slot 3 must change slot 3"
    _same(_run(p, g, 40), scalar, "set_prox(g) after a per-signal call")
    assert p.get_prox_params().tolist() == [lam] * 4


def test_a_column_of_a_path_is_that_penalty_s_own_solve(L, lpv2112):
    """Y = tile(y, 4) and four group-lasso penalties: column q of the path run equals, bit for bit, column q of a run of the same handle with
    the scalar lambda_q -- 60 iterations, across the correction of handles with several right-hand sides at iteration 16."""
    _, pt, Nf, Nv = lpv2112
    lmax = L.lambda_max(pt, L.SlicedSeparableSum, group_len=2 * Nv)
    assert np.all(lmax == lmax[0])
    lams = L.lambda_grid(float(lmax[0]), 4, ratio=0.05)
    gs = [L.SlicedSeparableSum.frequency_groups(l, Nf, 2 * Nv) for l in lams]
    path = _run(pt, gs, 60)
    assert pt.matvec_info()["kernel"] == WS and pt.timing()["xcorr_count"] >= 1, "the run must cross a correction"
    assert pt.get_prox_params().tolist() == lams.tolist()
    nnz = [int(np.count_nonzero(path[0][1][:, q])) for q in range(4)]
    assert nnz[0] < nnz[-1], ("the columns of a path must differ", nnz)
    for q in range(4):
        single = _run(pt, gs[q], 60)
        for nm, a, b in zip("xzu", path[0], single[0]):
            assert np.array_equal(a[:, q], b[:, q]), (f"column {q}, lambda = {lams[q]!r}", nm, int((a[:, q] != b[:, q]).sum()),
                                                       float(np.abs(a[:, q] - b[:, q]).max()))
        assert path[1][q] == single[1][q], (q, path[1][q], single[1][q])


# ---- 4. create_path from every constructor ----------------------------------------------------------------------------------------------------
def _fourier_data(zerofreq, weighted):
    rng = np.random.default_rng(11 + 2 * zerofreq + weighted)
    N, Nf = 400, 100
    t = np.sort(rng.random(N) * 10.0)
    f = (np.arange(Nf) + (0 if zerofreq else 1)) * 0.11
    y = 2 * np.cos(2 * np.pi * f[7] * t) + np.sin(2 * np.pi * f[31] * t + 0.3) + 0.5 * zerofreq + 0.1 * rng.standard_normal(N)
    W = 0.5 + rng.random(N) if weighted else None
    return y, t, f, W


def _small_lpv_data():
    rng = np.random.default_rng(3)
    N, Nv = 400, 8
    X = np.sort(10 * rng.random(N)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * np.arange(2, 28, 2.0)                                                # Nf = 13: n = 208
    y = 2 * V ** 2 * np.cos(w[0] * X) + 3 * np.exp(-10 * (V - 0.5) ** 2) * np.cos(w[9] * X) + 0.1 * rng.standard_normal(N)
    return y, X, V, w, Nv


def _dense_data():
    rng = np.random.default_rng(4)
    A = np.asfortranarray(rng.standard_normal((400, 200)))
    y = A[:, [3, 77, 150]] @ np.array([2.0, -1.5, 1.0]) + 0.1 * rng.standard_normal(400)
    return A, y


CONSTRUCTORS = ["fourier", "fourier-zerofreq", "fourier-W", "fourier-zerofreq-W", "lpv", "dense", "gram"]
ITERS = 150


def _source_and_single(L, ctor, kw):
    """(source handle, linear sign, prox of lambda, the single-signal estimator: lambda -> what `column` extracts, column: path handle -> [*, ns])."""
    LS, QW = 1, -1
    if ctor.startswith("fourier"):
        y, t, f, W = _fourier_data("zerofreq" in ctor, ctor.endswith("W"))
        return (L.Problem.fourier(y, t, f, W), QW if W is not None else LS, L.NormL1,
                lambda lam: L.ls_sparse_spectral(y, t, f, W, λ=lam, **kw)[0], lambda p: p.params(0),
                lambda lams: L.ls_sparse_spectral_path(y, t, f, W, λs=lams, **kw)[0])
    if ctor == "lpv":
        y, X, V, w, Nv = _small_lpv_data()
        return (L.Problem.lpv(y, X, V, w, Nv), LS, lambda lam: L.SlicedSeparableSum.frequency_groups(lam, len(w), 2 * Nv),
                lambda lam: L.ls_sparse_spectral_lpv(y, X, V, w, Nv, λ=lam, **kw).x, lambda p: p.params(0),
                lambda lams: np.stack([se.x for se in L.ls_sparse_spectral_lpv_path(y, X, V, w, Nv, λs=lams, **kw)], axis=1))
    A, y = _dense_data()
    z_of = lambda p: p.admm_get()[1]
    admm_kw = {k: v for k, v in kw.items() if k != "iteration"}
    if ctor == "dense":
        def single(lam):
            with L.default_options(iteration=kw.get("iteration")):
                return L.ADMM(np.zeros(200), L.LeastSquares(A, y), L.NormL1(lam), **admm_kw)[1]
        return L.Problem.dense(A, y), LS, L.NormL1, single, z_of, None
    G, b = A.T @ A, A.T @ y

    def single(lam):                                                                   # (Quadratic(Q, q): (Q + I/mu) x = v/mu - q)
        with L.default_options(iteration=kw.get("iteration")):
            return L.ADMM(np.zeros(200), L.Quadratic(G, -b), L.NormL1(lam), **admm_kw)[1]
    return L.Problem.gram(G, -b), QW, L.NormL1, single, z_of, None


@pytest.mark.parametrize("iteration", ["two", None], ids=["two-launch", "default"])
@pytest.mark.parametrize("ctor", CONSTRUCTORS)
def test_create_path_from_every_constructor(L, ctor, iteration):
    kw = dict(iters=ITERS, tol=0.0, printerval=10 ** 6, iteration=iteration)
    src, sign, make, single, column, path_estimator = _source_and_single(L, ctor, kw)
    G0, b0 = src.get_gram()
    n = src.n
    assert 190 <= n <= 210 and src.ns == 1
    gl = 16 if ctor == "lpv" else 0
    bmax = float(np.sqrt((b0.reshape(-1, gl) ** 2).sum(axis=1)).max()) if gl else float(np.abs(b0).max())
    if not ctor.endswith("W"):
        assert np.isclose(L.lambda_max(src, L.SlicedSeparableSum if gl else L.NormL1, group_len=gl), bmax, rtol=1e-14, atol=0.0)
    lams = 0.8 * L.lambda_grid(bmax, 3, ratio=0.04)[::-1]                               # ascending (column 0 is the densest), all below lambda_max
    src.set_option("iteration", iteration)                                             # (the path handle takes the source's options)
    path = L.Problem.path(src, 3)
    src.close()                                                                        # destroying the source first changes nothing
    with path:
        assert (path.n, path.ns, path.kind, path.f32) == (n, 3, src.kind, False) and path.get_option("iteration") == iteration
        Gp, bp = path.get_gram()
        assert np.array_equal(Gp, G0) and np.array_equal(bp, b0), "the Gram of the path handle must be the source's bits"
        B = path.get_rhs()
        assert B.shape == (n, 3) and all(np.array_equal(B[:, q], b0) for q in range(3)), "every right-hand side must be the source's"
        path.set_prox([make(l) for l in lams])
        path.admm_init(None, μ=0.05, tol=0.0, linear_sign=sign)
        info = path.matvec_info()
        assert info["kernel"] == (BATCH if iteration == "two" else SMALL), info
        path.admm_run(ITERS)
        cols = column(path).reshape(-1, 3, order="F")
    if path_estimator is not None:
        assert np.array_equal(path_estimator(lams), cols), "the path estimator is Problem.path + set_prox(list) + the existing driver"
    nnz = [int(np.count_nonzero(cols[:, q])) for q in range(3)]
    assert nnz[0] > nnz[2] > 0, ("the penalties must tell the columns apart", nnz)
    for q in range(3):
        ref = np.asarray(single(float(lams[q])))
        assert np.any(ref)
        if iteration == "two":
            assert np.array_equal(cols[:, q], ref), (ctor, q, int((cols[:, q] != ref).sum()), float(np.abs(cols[:, q] - ref).max()))
        else:
            rel = float(np.linalg.norm(cols[:, q] - ref) / np.linalg.norm(ref))
            print(f"[create_path {ctor} default route] column {q}: rel {rel:.3e}")
            assert rel <= 1e-11, (ctor, q, rel)


def test_r_path_through_the_estimator(L):
    """proxg=[IndBallL0(4), IndBallL0(8), ...]: an r-path; every estimate has at most r non-zero parameters and is the single estimator's."""
    y, t, f, _ = _fourier_data(False, False)
    kw = dict(iters=ITERS, tol=0.0, printerval=10 ** 6, iteration="two")
    params, fo, rs = L.ls_sparse_spectral_path(y, t, f, proxg=[L.IndBallL0(4), L.IndBallL0(8), L.IndBallL0(400)], **kw)
    assert params.shape == (100, 3) and rs.tolist() == [4.0, 8.0, 400.0] and np.array_equal(fo, f)
    for q, r in enumerate((4, 8, 400)):
        assert 0 < np.count_nonzero(params[:, q]) <= r
        assert np.array_equal(params[:, q], L.ls_sparse_spectral(y, t, f, proxg=L.IndBallL0(r), **kw)[0])


def test_path_estimators_default_grid(L):
    y, X, V, w, Nv = _small_lpv_data()
    ses = L.ls_sparse_spectral_lpv_path(y, X, V, w, Nv, nλ=4, iters=ITERS, tol=0.0, printerval=10 ** 6)
    with L.Problem.lpv(y, X, V, w, Nv) as src:
        grid = L.lambda_grid(L.lambda_max(src, L.SlicedSeparableSum, group_len=2 * Nv), 4)
    assert np.allclose([se.λ for se in ses], grid, rtol=1e-12, atol=0.0) and all(se.x.shape == (len(w) * Nv,) for se in ses)
    assert np.count_nonzero(ses[0].x) < np.count_nonzero(ses[-1].x), "lambda_max against a thousandth of it"
    y, t, f, W = _fourier_data(False, True)
    with pytest.raises(ValueError):
        L.ls_sparse_spectral_path(y, t, f, W)                                          # no lambda_max for the as-written weighted form
    params, _, lams = L.ls_sparse_spectral_path(y, t, f, nλ=3, iters=ITERS, tol=0.0, printerval=10 ** 6)
    assert params.shape == (100, 3) and lams.shape == (3,) and np.count_nonzero(params[:, 0]) < np.count_nonzero(params[:, 2])


# ---- 5. lambda_max on the device --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["l1-fourier", "group-lpv"])
def test_lambda_max_on_the_device(L, form):
    if form == "l1-fourier":
        rng = np.random.default_rng(5)
        N, Nf = 400, 40
        t = np.sort(rng.random(N) * 10.0)
        f = np.arange(1, Nf + 1) * 0.25
        y = 2 * np.cos(2 * np.pi * f[3] * t) + np.sin(2 * np.pi * f[20] * t + 0.3) + 0.1 * rng.standard_normal(N)
        src, kind, gl, make = L.Problem.fourier(y, t, f), L.NormL1, 0, L.NormL1
    else:
        y, X, V, w, Nv = _small_lpv_data()
        src, kind, gl = L.Problem.lpv(y, X, V, w, Nv), L.SlicedSeparableSum, 2 * Nv
        make = lambda lam: L.SlicedSeparableSum.frequency_groups(lam, len(w), gl)
    with src:
        lmax = L.lambda_max(src, kind, group_len=gl)
        assert isinstance(lmax, float) and lmax > 0
        with L.Problem.path(src, 2) as p:
            p.set_prox([make(1.01 * lmax), make(0.9 * lmax)])
            p.admm_init(None, μ=0.05, tol=1e-9)
            p.admm_run(20000)
            _, z, _ = p.admm_get()
            st = [p.admm_status(q) for q in range(2)]
    assert not np.any(z[:, 0]), ("1.01 lambda_max must give z = 0 exactly", int(np.count_nonzero(z[:, 0])))
    assert np.any(z[:, 1]), "0.9 lambda_max must leave a non-zero z"
    assert st[0][2] and st[1][2], ("both columns must have converged", st)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(L, handles):
    from lpvspectral_jl_amd import _lib
    lib = _lib.lib()
    p = handles(130, 3)
    good = [4.0, 8.0, 0.0]
    p.set_prox_params(P.L1, good)

    def raw(kind, vals, gl=0, count=None):
        a = np.ascontiguousarray(np.asarray(vals, dtype=np.float64))
        return lib.lpvs_problem_set_prox_per_signal(p._h, kind, _lib.out_ptr(a), len(vals) if count is None else count, gl)

    assert raw(P.L1, [1.0, 2.0]) == _lib.LPVS_EARGUMENT                                 # wrong count
    assert raw(P.L1, [1.0, 2.0, 3.0, 4.0]) == _lib.LPVS_EARGUMENT
    assert raw(P.L1, [1.0, -2.0, 3.0]) == _lib.LPVS_EARGUMENT                           # negative
    assert raw(P.L1, [1.0, 2.0, float("nan")]) == _lib.LPVS_EARGUMENT                   # not finite
    assert raw(P.L0, [float("inf"), 2.0, 3.0]) == _lib.LPVS_EARGUMENT
    assert raw(7, [1.0, 2.0, 3.0]) == _lib.LPVS_EUNSUPPORTED                            # the checks of lpvs_problem_set_prox
    assert raw(P.GROUP, [1.0, 2.0, 3.0], gl=0) == _lib.LPVS_EARGUMENT
    assert raw(P.GROUP, [1.0, 2.0, 3.0], gl=8193) == _lib.LPVS_EUNSUPPORTED
    out = np.zeros(4)
    assert lib.lpvs_problem_get_prox_params(p._h, _lib.out_ptr(out), 4) == _lib.LPVS_EARGUMENT
    assert p.get_prox_params().tolist() == good, "a refused call must change nothing"
    with pytest.raises(ValueError):
        p.set_prox([L.NormL1(1.0), L.NormL1(2.0)])                                      # wrong count through the list
    with pytest.raises(ValueError):
        p.set_prox([L.NormL1(1.0), L.NormL0(2.0), L.NormL1(3.0)])                       # mixed kinds
    with pytest.raises(ValueError):
        p.set_prox([L.SlicedSeparableSum.frequency_groups(1.0, 13, 10), L.SlicedSeparableSum.frequency_groups(1.0, 10, 13),
                    L.SlicedSeparableSum.frequency_groups(1.0, 13, 10)])                # mixed group lengths
    with pytest.raises(NotImplementedError):
        p.set_prox([L.NormL1(1.0), object(), L.NormL1(3.0)])
    h = C.c_void_p()
    assert lib.lpvs_problem_create_path(p._h, 2, C.byref(h)) == _lib.LPVS_EARGUMENT and not h.value   # a source with several signals
    with L.Problem.gram(np.eye(5, order="F"), np.ones(5)) as src:
        for ns in (0, -1, 65):
            assert lib.lpvs_problem_create_path(src._h, ns, C.byref(h)) == _lib.LPVS_EARGUMENT and not h.value
        with pytest.raises(ValueError):
            L.Problem.path(src, 65)
        with L.Problem.path(src, 64) as p64, L.Problem.path(src, 1) as p1:
            assert (p64.ns, p1.ns) == (64, 1) and p64.get_rhs().shape == (5, 64)
            p1.set_prox([L.NormL1(0.5)])                                                # one slot: the scalar
            assert p1.get_prox_params().tolist() == [0.5]
    assert p.get_prox_params().tolist() == good
    rng = np.random.default_rng(6)
    v, _ = P.cuts(130, rng, 0.25)
    Z0 = _slots(3, lambda q: v)
    run_case(p, SMALL, P.L1, good, 0, 2.0 ** -4, Z0, np.zeros_like(Z0), label="after the refused calls")
