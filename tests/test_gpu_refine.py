"""The accurate linear algebra of csrc/admm_refine.hip -- the refined ridge solve, the offset vector refined against a Dot2 residual, the x-update
correction -- held in isolation to the exact-arithmetic bounds of tests/_refine_ref.py (derived there) on a family whose H, b and x*
are doubles without rounding and whose cond(H) is 2^20 exactly.  GPU only.

Every input of a bound is computed on the host from the device's OWN inverse (get_inverse(shift)); the residuals are exact (integers, rounded once).
tests/test_refine_ref_host.py shows that the same recurrences with a residual formed in plain doubles, or in x87 long doubles, or with no refinement,
miss these bounds by factors of 1e3 .. 1e7: a compensation term lost in the wave shuffle, fused error-free transformations, x read from the wrong
signal in the second group of eight, or pad rows entering a sum at n < np would turn these tests red.

The ABI hands out the n valid entries of the offset vector and of the solution and nothing of the pad: no pad entry is observable here; what a wrong
pad could do to the valid rows is inside the bounds at n = 2100 (np = 2176)."""
import numpy as np
import pytest

import _packed_ref as PR
import _refine_ref as R

pytestmark = pytest.mark.gpu

MU = 1.0               # shift = 1/mu = 1: the handle's Gram is G = H - I


def _ld(a):
    return np.asarray(a).astype(np.longdouble)


@pytest.fixture(scope="module")
def cases(L):
    """Per n: the family, a gram handle on (G, b), the device's inverse as the kernels read it and what the bounds need of it."""
    cache = {}

    def get(n):
        if n not in cache:
            F = R.family(n)
            p = L.Problem.gram(F.G, F.b[:, 0])
            A = np.ascontiguousarray(p.get_inverse(1.0 / MU).T)               # device row-major: A[r, c] = M[r][c]
            cache[n] = (F, p, R.Inverse(F, A))
        return cache[n]
    yield get
    for _, p, _ in cache.values():
        p.close()


def _offsets(L, p, monkeypatch, correction="off", sign=None):
    """(xb0 = fl(M b), xb1 = the refined one) of a handle on 8-byte tiles: two lpvs_admm_init, the first with LPVS_XB_REFINE=0."""
    p.set_option("storage", "f64")                     # the offset is n values per signal, no nibble term rides in it
    p.set_option("xupdate_correction", correction)
    p.set_prox(L.NormL1(1.0))
    out = []
    for steps in ("0", None):
        if steps is None:
            monkeypatch.delenv("LPVS_XB_REFINE", raising=False)
        else:
            monkeypatch.setenv("LPVS_XB_REFINE", steps)
        p.admm_init(None, μ=MU, tol=0.0, **({} if sign is None else dict(linear_sign=sign)))
        xb = p.admm_get_offset()
        assert xb is not None and xb.size == p.n * p.ns
        out.append(xb.reshape(p.n, p.ns, order="F"))
    return out


def _require_an_inverse(inv, label):
    if not inv.normE < 2.0 ** -16:
        pytest.fail(f"{label}: |I - M H|_inf = {inv.normE:.3e} >= 2^-16: the factorisation is wrong", pytrace=False)


def _hold_offset(F, inv, b, xstar, xb0, xb1, label):
    """One column: xb0 a rounded product, xb1 within both bounds; -> (product, model, forward) ratios."""
    rp = R.worst_ratio(_ld(xb0) - inv.Ald @ _ld(b), R.product_bound(F, inv, b))
    m = R.offset_model(F, inv, b, xb0)
    rm = R.worst_ratio(_ld(xb1) - m["xb1"], m["bound"])
    rf = R.worst_ratio(xb1 - xstar, R.offset_forward_bound(F, inv, xb0, xstar, m["bound"]))
    print(f"[refine] {label}: |E|_inf {inv.normE:.2e}; M b / bound {rp:.3e}; refined offset vector / bound: vs the exact step {rm:.3e}, vs x* {rf:.3e} "
          f"(max|xb0 - x*| {np.abs(xb0 - xstar).max():.2e}, max|xb1 - x*| {np.abs(xb1 - xstar).max():.2e}, bound {m['bound'].max() / (8 * R.U):.2f} u max|x*|)")
    assert rp <= 1, (label, "M b", rp)
    assert rm <= 1 and rf <= 1, (label, "refined", rm, rf)
    return rp, rm, rf


@pytest.mark.parametrize("n", R.OFFSET_SIZES)
def test_offset_vector_is_one_exact_refinement_step(L, cases, monkeypatch, n):
    F, p, inv = cases(n)
    _require_an_inverse(inv, f"n = {n}")
    xb0, xb1 = _offsets(L, p, monkeypatch)
    assert not np.array_equal(xb0, xb1)
    _hold_offset(F, inv, F.b[:, 0], F.xstar[:, 0], xb0[:, 0], xb1[:, 0], f"offset vector n = {n} (np = {R.padded_size(n)})")


def test_offset_vector_of_the_negated_linear_term_is_the_negative(L, cases, monkeypatch):
    F, p, inv = cases(2100)
    plus = _offsets(L, p, monkeypatch)
    minus = _offsets(L, p, monkeypatch, sign=-1)                                # (LINEAR_QUADRATIC_AS_WRITTEN: the linear term enters negated)
    for a, b in zip(plus, minus):
        assert np.any(a) and np.array_equal(-a, b)


# ---- nine right-hand sides: two signal groups (8 + 1) in shifted_residual_dd_kernel and symv_rows_multi_kernel<8> ---------------------------
NS = 9


@pytest.fixture(scope="module")
def nine(L):
    """An lpv_multi handle of n = 2 Nf Nv = 2048 whose Gram and nine right-hand sides are overwritten by the family's."""
    import torch
    Nf, Nv, N = 128, 8, 4096
    rng = np.random.default_rng(9)
    X = np.sort(rng.random(N) * (10.0 * N / 500)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    F = R.family(2048, NS)
    assert len({tuple(c) for c in F.xstar.T}) == NS
    p = L.Problem.lpv_multi(np.asfortranarray(rng.standard_normal((N, NS))), X, V, w, Nv)
    assert p.n == 2048 and p.ns == NS
    Gt, bt = p.device_gram()
    assert tuple(Gt.shape) == (2048, 2048) and tuple(bt.shape) == (NS, 2048)
    Gt.copy_(torch.from_numpy(F.G))
    bt.copy_(torch.from_numpy(np.ascontiguousarray(F.b.T)))
    torch.cuda.synchronize()
    p.gram_modified()
    A = np.ascontiguousarray(p.get_inverse(1.0 / MU).T)
    yield F, p, R.Inverse(F, A)
    p.close()


def test_offset_vectors_of_nine_right_hand_sides(L, nine, monkeypatch):
    F, p, inv = nine
    _require_an_inverse(inv, "nine right-hand sides")
    xb0, xb1 = _offsets(L, p, monkeypatch)
    worst = np.zeros(3)
    for q in range(NS):
        worst = np.maximum(worst, _hold_offset(F, inv, F.b[:, q], F.xstar[:, q], xb0[:, q], xb1[:, q], f"nine right-hand sides, column {q}"))
    print(f"[refine] nine right-hand sides, worst over the columns: M b {worst[0]:.3e}, vs the exact step {worst[1]:.3e}, vs x* {worst[2]:.3e}")
    # admm_refine.hip: per signal the arithmetic of symv_rows_multi_kernel is symv_kernel<1>'s operation for operation (lane j takes the column pairs
    # j, j + 64, ... in order, two fma per pair, then the same shuffle sum), and a signal's Dot2 accumulator never meets another's: column q is the
    # single-signal handle's offset vector for b_q BIT FOR BIT -- given the same inverse, which the same Gram through the same sweep is.
    with L.Problem.gram(F.G, F.b[:, 0]) as one:
        A1 = np.ascontiguousarray(one.get_inverse(1.0 / MU).T)
        if not np.array_equal(A1, inv.A):
            pytest.fail("the single-signal handle's inverse of the same Gram differs from the nine-signal handle's: nothing to compare bit for bit", pytrace=False)
        _, b1 = one.device_gram()
        import torch
        for q in range(NS):
            b1[0].copy_(torch.from_numpy(F.b[:, q].copy()))
            torch.cuda.synchronize()
            one.gram_modified()
            s0, s1 = _offsets(L, one, monkeypatch)
            assert np.array_equal(s0[:, 0], xb0[:, q]), ("M b", q, float(np.abs(s0[:, 0] - xb0[:, q]).max()))
            assert np.array_equal(s1[:, 0], xb1[:, q]), ("refined", q, float(np.abs(s1[:, 0] - xb1[:, q]).max()))


# ---- the refined ridge solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.RIDGE_SIZES)
def test_ridge_solve_residual_is_within_its_bound(L, cases, n):
    F, p, inv = cases(n)
    _require_an_inverse(inv, f"n = {n}")
    b, xstar = F.b[:, 0], F.xstar[:, 0]
    x = p.solve_ridge(1.0 / MU)
    r2 = R.exact_residual(F, b, x)[0]
    xs = R.ridge_recurrence(F, inv, b, 2)                                       # the same recurrence in host doubles: r1 is not observable
    r1 = R.exact_residual(F, b, xs[1])[0]
    ratio = R.worst_ratio(r2, R.ridge_residual_bound(F, inv, b, x, r1))
    r0 = R.exact_residual(F, b, xs[0])[0]
    none = R.worst_ratio(r0, R.ridge_residual_bound(F, inv, b, xs[0], r1))
    fwd, fwd_bound = float(np.abs(x - xstar).max()), float((inv.absA @ np.abs(r2)).max())
    print(f"[refine] ridge solve n = {n}: |E|_inf {inv.normE:.2e}; exact residual / bound {ratio:.3e} (M b alone on the host: {none:.3g}); rel residual "
          f"{np.linalg.norm(r2) / np.linalg.norm(b):.2e}; max|x - x*| {fwd:.2e} <= max |M||r| {fwd_bound:.2e}")
    assert ratio <= 1, (n, ratio)
    assert fwd <= fwd_bound, (n, fwd, fwd_bound)


def _host_two_steps(H, b):
    """Relative residual after two plain-double steps with numpy's inverse (what lpvs_problem_solve_ridge tests against 1e-9), and the spectrum's ends."""
    n = len(b)
    G = H - np.eye(n)
    assert np.array_equal(G + np.eye(n), H)                                     # what the device factors is H itself
    A = np.linalg.inv(H)
    x = A @ b
    for _ in range(2):
        x = x + A @ (b - (G @ x + x))
    ev = np.linalg.eigvalsh(H)
    return G, float(np.linalg.norm(b - (G @ x + x)) / np.linalg.norm(b)), float(ev[0]), float(ev[-1])


def test_ridge_solve_refuses_for_its_residual(L):
    """lpvs_problem_solve_ridge's own refusal, `relative residual > 1e-9 after refinement`: d over [1, 2^36] at n = 200 and b = x* the eigenvector of
    d = 1 (tests/_refine_ref.eigenvector_rhs).  gamma_n |H|_2 = 1.6e-3 < lambda_min = 1: no pivot can be lost, the factorisation must go through; the
    residual in doubles cannot fall below the rounding of H x, 3e-6 of |b| on the host -- so the message is the residual test's and nothing else."""
    H, b = R.eigenvector_rhs()
    G, rel, lmin, lmax = _host_two_steps(H, b)
    print(f"[refine] residual refusal: host relative residual after two steps {rel:.2e}; lambda_min {lmin:.3g}, gamma_n |H|_2 {R.gamma(len(b)) * lmax:.3g}")
    assert lmin > 100 * R.gamma(len(b)) * lmax and rel > 1e-7
    with L.Problem.gram(G, b) as p:
        with pytest.raises(L.NumericError, match="too ill-conditioned.*relative residual") as ei:
            p.solve_ridge(1.0)
        print(f"[refine] residual refusal: {ei.value}")
        rep = float(str(ei.value).split("relative residual")[1].split()[0])
        assert 1e-9 < rep < 1e-3, rep                                           # (the figure it reports is a residual of this size, not a NaN or a blow-up)


def test_ridge_solve_refuses_a_spectrum_it_cannot_refine(L):
    """d over [1, 2^50] at n = 200 with a generic b = H x*: NumericError, by either refusal.  For a GENERIC right-hand side the residual refusal sets in
    where refinement in doubles stalls, cond(H) n u ~ 1, which is also where an elimination without pivoting loses the guarantee of positive pivots
    (gamma_n |H|_2 = 27 against lambda_min = 0.98 here; the exact pivots are >= 25).  LAPACK's Cholesky goes through and the host recurrence leaves a
    residual of 2e-7 (the residual refusal); the device's block sweep, which eliminates with explicit inverses of its 64-wide diagonal blocks, meets a
    non-positive pivot (MI355X).  Both are right answers; the residual refusal has its own case above."""
    H, b = R.hopeless()
    G, rel, lmin, lmax = _host_two_steps(H, b)
    print(f"[refine] refusal: host relative residual after two steps {rel:.2e}; lambda_min {lmin:.3g}, gamma_n |H|_2 {R.gamma(len(b)) * lmax:.3g}")
    assert rel > 1e-9 and lmin < R.gamma(len(b)) * lmax                         # refused on the host for its residual; pivots not guaranteed
    with L.Problem.gram(G, b) as p, pytest.raises(L.NumericError) as ei:
        p.solve_ridge(1.0)
    msg = str(ei.value)
    print(f"[refine] refusal: {msg}")
    assert ("too ill-conditioned" in msg and "relative residual" in msg) or "non-positive pivot" in msg, msg


# ---- the x-update correction -------------------------------------------------------------------------------------------------------------------
def _hold_correction(L, F, p, inv, monkeypatch, label):
    """lpvs_admm_set_state(iters_done = 1) runs launch_xupdate_correction at once on v = (z - u) / mu as admm_restate_kernel forms it."""
    n, ns = p.n, p.ns
    xb0 = _offsets(L, p, monkeypatch, correction="on")[1]                        # (the handle is left initialised with the refined vector: xb0)
    Mt = PR.packed_model(inv.A, n, ns=ns, storage="f64")["Mt"]                   # 8-byte tiles: the lower triangle, mirrored
    invt = inv if np.array_equal(Mt, inv.A) else R.Inverse(F, Mt)
    rng = np.random.default_rng(40 + ns)
    V = rng.integers(-8, 9, (n, ns)).astype(np.float64)                          # small integers: |M||v| stays near |M v|
    Uu = rng.integers(-5, 6, (n, ns)).astype(np.float64)
    Z = V + Uu
    assert np.array_equal((Z - Uu) / MU, V)
    shape = (lambda a: np.asfortranarray(a) if ns > 1 else a[:, 0])
    p.admm_set_state(shape(np.zeros((n, ns))), shape(Z), shape(Uu), iters=1)
    xbe = p.admm_get_offset().reshape(n, ns, order="F")
    worst = np.zeros(2)
    for q in range(ns):
        m = R.correction_model(F, invt, V[:, q], xb0[:, q])
        got = _ld(xbe[:, q]) - _ld(xb0[:, q])
        rw, rt = R.worst_ratio(got - m["d"], m["bound"]), R.worst_ratio(got - m["d"], m["bound_tight"])
        rz = R.worst_ratio(m["d"], m["bound_tight"])
        print(f"[refine] {label}, column {q}: max|d| {float(np.abs(m['d']).max()):.2e}; (xb_eff - xb0) - d over the bound {rw:.3e}, over the tight bound {rt:.3e} "
              f"(d = 0 would give {rz:.3g})")
        assert rw <= 1 and rt <= 1, (label, q, rw, rt)
        assert np.any(got != 0)
        worst = np.maximum(worst, (rw, rt))
    return worst


def test_xupdate_correction_single_signal(L, cases, monkeypatch):
    F, p, inv = cases(2100)
    _require_an_inverse(inv, "n = 2100")
    _hold_correction(L, F, p, inv, monkeypatch, "correction n = 2100")


def test_xupdate_correction_nine_signals(L, nine, monkeypatch):
    F, p, inv = nine
    _require_an_inverse(inv, "nine right-hand sides")
    w = _hold_correction(L, F, p, inv, monkeypatch, "correction, nine signals")
    print(f"[refine] correction, nine signals, worst over the columns: {w[0]:.3e} (bound), {w[1]:.3e} (tight bound)")
