"""Shared by tests/test_dense_ref_host.py and tests/test_gpu_dense_estimators.py: the componentwise backward error the dense estimators
(ls_spectral tall / fat / weighted, ls_spectral_lpv, the dense estimator of the window engine) are held to, the extended-precision solutions
for the outputs whose coefficients are not observable, the host restatements of fva and of the un-permutation of Sigma, and the case tables.

The metric.  A path that solves H x = b, H = Phi' diag(W) Phi + rho I, b = Phi' (W .* y), is judged on the regressor Phi the library itself
materialises (doubles, taken as exact).  In long double, every product and sum from Phi, W, y and nothing rounded in between:

    r = Phi' (W .* (y - Phi x^)) - rho x^ ,        omega(x^) = max_i |r_i| / ((E |x^|)_i + f_i) ,
    E = B_G + c_s gamma_(np+2) |H| ,               f = B_b + c_s gamma_(np+2) |b| ,        gamma_k = k u / (1 - k u), u = 2^-53,

np the padded order (a multiple of 128) of the system the device solves.  An output passes when omega <= 1: every entry, none exempt.  The
metric does not grow with cond(H): a backward-stable solve of the device's own system sits far below 1 whatever the conditioning, an explicit
inverse applied without refinement sits cond(H) u / gamma above it.

B_G, B_b: what the device's Gram and right-hand side may differ from the exact ones by, entrywise, as the project states it for the form that ran
(tests/_gram_ref.py): the dense forms (panel, kr, krs) (N + 16) u S and (N + 16) u s with S = sum_k |W_k Phi_ka Phi_kb|, s = sum_k |W_k Phi_ka y_k|
from oracle.gram_ld; the structured forms (ap, ap-nufft) struct_tol(max|w|, max|x|) times the weight sum of the activation pair, C[j][j'] =
sum_k |W_k K_kj K_kj'| (Fourier: sum_k |W_k| / (2 Nf)), and times sum_k |W_k K_kj y_k| for b (Fourier: sum_k |W_k y_k| / sqrt(2 Nf)).  With
H_dev = H + dG, b_dev = b + db:  b - H x^ = (b_dev - H_dev x^) + (dG x^ - db), and |dG x^ - db| <= B_G |x^| + B_b.

c_s.  What is left is the residual of the device's own system after fixed-precision iterative refinement with the residual formed in doubles
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 12.2, Theorem 12.4; Skeel 1980).  One round is
    r^ = fl(b - H x^) = b - H x^ + dr,   |dr| <= gamma_(np+2) (|b| + |H| |x^|)     (np products and sums in any order, the ridge fma, the subtraction)
    d^ = M r^ (+ its own error),         x+ = fl(x^ + d^) = x^ + d^ + e,  |e| <= u |x+| .
Then  b - H x+ = (b - H x^ - r^) + (r^ - H d^) - H e = -dr + (I - H M) r^ + (second order) - H e.  At convergence |(I - H M) r^| is of second order
(r^ is itself O(gamma) and |I - H M| < 1 is what convergence means), x^ and x+ agree to first order, and
    |b - H x+| <= gamma_(np+2) (|b| + |H| |x+|) + u |H| |x+| + O(u^2)  <=  2 gamma_(np+2) (|b| + |H| |x+|) :
c_s = 2, Higham's constant (his gamma_(n+1) counts a residual without the ridge term).  Derived, not measured; LAPACK's solve of the same H, b
sits at 1e-5 .. 1e-2 of the resulting bound (tests/test_dense_ref_host.py prints every figure), the explicit inverse without refinement at
cond(H) ~ 1e10 on the dense Gram forms five decades above it.

The dual form (fat ls_spectral: alpha = (A A' + lam^2 I)^-1 y, x = A' alpha) is held to the SAME primal-form omega with rho = lam^2, W = 1, the
dense-form Gram bounds of the primal Gram and np the padded order of the dual system.  An exact dual solution has r = 0; a dual solution with
residual r_d has r = A' r_d.  Where the primal-form omega of the refined dual emulation in doubles exceeds 1/4 the case does not belong here but
to the refusal group (checked on the host).

Outputs whose x is not observable (S of lpvs_windowpsd_lpv_f64, the csd accumulators, Sigma) are held to the first-order forward bound
|x^ - x*| <= |M| (E |x*| + f), M = H^-1 in extended precision (oracle.inverse_ld): x^ solves (H + dH) x^ = b + db with |dH| <= E, |db| <= f when
omega <= 1 (Oettli-Prager), and x^ - x* = -M (dH x^ - db) to first order."""
import numpy as np

import _gram_ref as GR
from oracle import oracle as O

U = 2.0 ** -53
LD = np.longdouble
C_S = 2.0
DENSE_FORMS = ("panel", "kr", "krs", "dense")
STRUCT_FORMS = ("ap", "ap-nufft")


def gamma(k):
    return k * U / (1 - k * U)


def padded(n):
    return -(-n // 128) * 128


# ---- Gram bounds of the form that ran ---------------------------------------------------------------------------------------------------
def fourier_pair_scale(Nf, n, y, W=None):
    """(C, c) of the structured Fourier form: the n x n weight sum sum_k |W_k| / (2 Nf) and sum_k |W_k y_k| / sqrt(2 Nf) per entry of b."""
    w = np.ones(len(y)) if W is None else np.abs(np.asarray(W, dtype=np.float64))
    return np.full((n, n), w.sum() / (2 * Nf)), np.full(n, float(np.sum(w * np.abs(y))) / np.sqrt(2 * Nf))


def lpv_pair_scale(K, Nf, y):
    """(C, c) of the structured LPV form in the permuted column order p = f 2 nb + c nb + j: C[j(a)][j(b)] = sum_k |K_kj K_kj'|, c = sum_k |K_kj y_k|."""
    K = np.abs(np.asarray(K, dtype=np.float64))
    nb = K.shape[1]
    j = np.arange(2 * Nf * nb) % nb
    return (K.T @ K)[np.ix_(j, j)], (K.T @ np.abs(y))[j]


def system(Phi, W, y, rho, form, nsolve=None, wmax=0.0, xmax=0.0, pair=None):
    """What omega and forward_bound share: dict(H |H| b E f n N) with G, b from oracle.gram_ld (long double sums, rounded once)."""
    Phi = np.asarray(Phi, dtype=np.float64)
    N, n = Phi.shape
    G, S, b, s = O.gram_ld(Phi, np.asarray(y, dtype=np.float64), W)
    if form in DENSE_FORMS:
        BG, Bb = GR.bound(N, S), GR.bound(N, s)
    elif form in STRUCT_FORMS:
        tol = GR.struct_tol(wmax, xmax)
        BG, Bb = tol * pair[0], tol * pair[1]
    else:
        raise ValueError(form)
    g = C_S * gamma(padded(n if nsolve is None else nsolve) + 2)
    absH = np.abs(G) + rho * np.eye(n)
    return dict(G=G, b=b, absH=absH, E=BG + g * absH, f=Bb + g * np.abs(b), n=n, N=N, rho=rho)


def fourier_system(A, t, f, y, W, rho, form, nsolve=None):
    """system() of a Fourier regressor A whose Gram ran as `form` ("dense" and "panel" alike: the panel kernel)."""
    if form in STRUCT_FORMS:
        return system(A, W, y, rho, form, nsolve=nsolve, wmax=6.283185307179586 * float(np.max(f)), xmax=float(np.max(np.abs(t))),
                      pair=fourier_pair_scale(len(f), A.shape[1], y, W))
    return system(A, W, y, rho, form, nsolve=nsolve)


def residual_ld(Phi, W, y, rho, x):
    """Phi' (W .* (y - Phi x)) - rho x in long double."""
    P = np.asarray(Phi, dtype=np.float64).astype(LD)
    w = np.ones(P.shape[0], dtype=LD) if W is None else np.asarray(W, dtype=np.float64).astype(LD)
    x = np.asarray(x, dtype=np.float64).astype(LD)
    return P.T @ (w * (np.asarray(y, dtype=np.float64).astype(LD) - P @ x)) - LD(rho) * x


def omega(Phi, W, y, rho, xhat, form, sys=None, **kw):
    """-> (worst ratio, its index, the ratios).  A non-finite x^ is infinitely wrong."""
    sys = system(Phi, W, y, rho, form, **kw) if sys is None else sys
    xhat = np.asarray(xhat, dtype=np.float64)
    if not np.all(np.isfinite(xhat)):
        return np.inf, int(np.argmin(np.isfinite(xhat))), np.full(sys["n"], np.inf)
    r = np.abs(residual_ld(Phi, W, y, rho, xhat)).astype(np.float64)
    den = sys["E"] @ np.abs(xhat) + sys["f"]
    assert np.all(den > 0)
    ratios = r / den
    return float(ratios.max()), int(np.argmax(ratios)), ratios


def solve_ld(sys):
    """x* = H^-1 b in extended precision as (hi, lo), and M = H^-1 rounded once (oracle.inverse_ld on the long-double Gram)."""
    M, hi, lo = O.inverse_ld(sys["G"], 1.0 / sys["rho"], sys["b"])
    return hi, lo, M


def forward_bound(sys):
    """-> (x* hi, x* lo, |M| (E |x*| + f)): first order, componentwise."""
    hi, lo, M = solve_ld(sys)
    return hi, lo, np.abs(M) @ (sys["E"] @ np.abs(hi) + sys["f"])


# ---- extended-precision least squares (the refusal group: no normal equations) ------------------------------------------------------------
def lstsq_ld(B, c):
    """min |B x - c| by Householder QR in long double (B tall, full column rank)."""
    R = np.array(B, dtype=LD)
    c = np.array(c, dtype=LD)
    m, n = R.shape
    for k in range(n):
        v = R[k:, k].copy()
        nv = np.sqrt(v @ v)
        if nv == 0:
            continue
        v[0] += nv if v[0] >= 0 else -nv
        v /= np.sqrt(v @ v)
        R[k:, k:] -= 2 * np.outer(v, v @ R[k:, k:])
        c[k:] -= 2 * v * (v @ c[k:])
    x = np.zeros(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        x[k] = (c[k] - R[k, k + 1:n] @ x[k + 1:]) / R[k, k]
    return x


def ridge_solution_ld(A, y, lam):
    """The minimiser of |A x - y|^2 + lam^2 |x|^2 through [A; lam I] in long double: cond(A), not its square."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    return lstsq_ld(np.vstack([A.astype(LD), LD(lam) * np.eye(n, dtype=LD)]), np.concatenate([np.asarray(y, dtype=np.float64).astype(LD), np.zeros(n, dtype=LD)]))


def fat_solution_ld(A, y, lam):
    """The same for N < nreg (what the dual form computes)."""
    assert A.shape[0] < A.shape[1]
    return ridge_solution_ld(A, y, lam)


def numpy_route(A, y, lam):
    """The reference's route in doubles: [A; lam I] \\ [y; 0] by LAPACK's SVD least squares."""
    n = A.shape[1]
    return np.linalg.lstsq(np.vstack([A, lam * np.eye(n)]), np.concatenate([y, np.zeros(n)]), rcond=None)[0]


def rel_l2(a, b):
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    return float(np.sqrt(np.sum(np.abs(a - b) ** 2) / np.sum(np.abs(b) ** 2)))


# ---- host emulations of the device's solves (doubles, numpy's LAPACK inverse in the place of the block sweep) -----------------------------
def refined(H, b, rounds):
    """x = M b and `rounds` rounds x += M (b - H x) with M = inv(H): launch_ridge_solve_refined / launch_batch_ridge_solve in host doubles."""
    M = np.linalg.inv(H)
    x = M @ b
    for _ in range(rounds):
        x = x + M @ (b - H @ x)
    return x


def normal_equations(Phi, W, y, rho):
    Phi = np.asarray(Phi, dtype=np.float64)
    WP = Phi if W is None else Phi * np.asarray(W)[:, None]
    return WP.T @ Phi + rho * np.eye(Phi.shape[1]), WP.T @ y


def dual_emulation(A, y, lam, rounds=2):
    """x = A' alpha, alpha the refined solve of (A A' + lam^2 I) alpha = y."""
    return A.T @ refined(A @ A.T + lam * lam * np.eye(A.shape[0]), y, rounds)


# ---- coefficient layouts ------------------------------------------------------------------------------------------------------------------
def complex2fourier(x, zero):
    """The inverse of fourier2complex (src/utilities.jl:62-73): [re; im], the sine of a leading zero frequency dropped."""
    x = np.asarray(x)
    return np.concatenate([x.real, x.imag[1:] if zero else x.imag]).astype(np.float64)


def fourier_regressor_np(t, f):
    """numpy statement of src/lsfft.jl:26-49 (host tests and the choice of inputs; the GPU tests take the library's own)."""
    t, f = np.asarray(t, np.float64), np.asarray(f, np.float64)
    dd = 1.0 / np.sqrt(2 * len(f))
    phi = (6.283185307179586 * f)[None, :] * t[:, None]
    c, s = np.cos(phi) * dd, -np.sin(phi) * dd
    return np.hstack([c, s[:, 1:]]) if f[0] == 0 else np.hstack([c, s])


def lpv_unpermutation(Nf, nb):
    """perm with reference order u = c Nf nb + j Nf + f  <-  device order p = f 2 nb + c nb + j (api.py: ls_spectral_lpv); restated with loops."""
    perm = np.empty(2 * Nf * nb, dtype=np.int64)
    for f in range(Nf):
        for c in range(2):
            for j in range(nb):
                perm[c * Nf * nb + j * Nf + f] = f * 2 * nb + c * nb + j
    return perm


def lpv_stats_ld(Phi, Y, x):
    """(var_e, var_y, fva) of src/lsfft.jl:252-255 in long double: e = Y - Phi x, corrected variances, fva = 1 - var(e) / var(Y)."""
    e = np.asarray(Y).astype(LD) - np.asarray(Phi).astype(LD) @ np.asarray(x).astype(LD)
    Yl = np.asarray(Y).astype(LD)
    N = len(Yl)
    var_e = np.sum((e - e.sum() / N) ** 2) / (N - 1)
    var_y = np.sum((Yl - Yl.sum() / N) ** 2) / (N - 1)
    return var_e, var_y, 1 - var_e / var_y


def sigma_ld(var_e, M, Nf, nb):
    """Sigma = var(e) P M P' (:253), M in the device's column order."""
    perm = lpv_unpermutation(Nf, nb)
    return LD(var_e) * np.asarray(M).astype(LD)[np.ix_(perm, perm)]


# ---- cases: ls_spectral --------------------------------------------------------------------------------------------------------------------
def _grid(nreg, zero, jitter, rng):
    """Nf frequencies in [0, 1/2) with nreg regressors: k / nreg (zero first) or (k + 1/2) / nreg -- the real Fourier basis of nreg integer stamps --
    moved by jitter x spacing (never the zero frequency): jitter = 0 is an arithmetic progression (structured Gram), else not (panel)."""
    Nf = (nreg + 1) // 2 if zero else nreg // 2
    f = (np.arange(Nf) + (0.0 if zero else 0.5)) / nreg
    if jitter:
        d = jitter * rng.uniform(-1, 1, Nf) / nreg
        d[0] = 0.0 if zero else d[0]
        f = f + d
    return f


# (id, nreg, zero frequency, N, weighted, lam, frequency jitter (0: progression -> ap), stamp jitter)
PRIMAL_CASES = [
    ("n127-N333", 127, True, 333, False, 1e-10, 0.3, 0.3),
    ("n128-N333", 128, False, 333, False, 1e-10, 0.3, 0.3),
    ("n129-N333", 129, True, 333, False, 1e-10, 0.3, 0.3),
    ("n257-N333", 257, True, 333, False, 1e-10, 0.3, 0.3),
    ("n127-N127", 127, True, 127, False, 1e-10, 0.3, 0.1),        # N = nreg: the boundary goes primal
    ("n128-N128", 128, False, 128, False, 1e-10, 0.3, 0.1),
    ("n129-N129", 129, True, 129, False, 1e-10, 0.3, 0.1),
    ("n257-N257", 257, True, 257, False, 1e-10, 0.3, 0.1),
    ("n129-N333-ap", 129, True, 333, False, 1e-6, 0.0, 0.3),      # progression: the structured form (lam = 1e-6: at 1e-10 its pair-scale bound
                                                                  # cannot tell lam from lam^2, omega 3.7 on the host)
    ("n127-N333-W", 127, True, 333, True, 1e-3, 0.3, 0.3),        # weighted: the ridge is lam
    ("n128-N333-W", 128, False, 333, True, 1e-3, 0.3, 0.3),
    ("n257-N333-W", 257, True, 333, True, 1e-10, 0.3, 0.3),
    ("n129-N333-W-ap", 129, True, 333, True, 1e-3, 0.0, 0.3),
]
PRIMAL = {c[0]: c for c in PRIMAL_CASES}


def primal_inputs(case):
    """(y, t, f, W, rho)"""
    cid, nreg, zero, N, weighted, lam, fj, tj = case
    rng = np.random.default_rng(31000 + 7 * nreg + N + int(weighted))
    t = np.arange(N) + tj * rng.random(N)
    f = _grid(nreg, zero, fj, rng)
    y = np.sin(2 * np.pi * f[len(f) // 3] * t) + 0.5 * rng.standard_normal(N) + (0.7 if zero else 0.0)
    W = 0.1 + rng.random(N) if weighted else None
    return y, t, f, W, (lam if weighted else lam * lam)


# (id, nreg, zero frequency, N, grade, stamp jitter delta): t = k + delta rand, lam = 1e-10.  Grade "well": cond(A A' + lam^2 I) in [1, 10];
# "mid": in [1e4, 1e7], where the explicit inverse alone misses; delta chosen on the host (among multiples of 1/16, one where the unrefined emulation
# misses by 30x and more and the refined one stays below 1/8 when the dual Gram is moved by an ulp: what LAPACK's inverse loses depends on its
# rounding, and another machine's rounds differently), test_dense_ref_host.py asserts the grade.
DUAL_CASES = [
    ("N=nreg-1", 101, True, 100, "well", 0.02),
    ("N=nreg-1", 101, True, 100, "mid", 1.9375),
    ("N=nreg-2", 102, False, 100, "well", 0.02),
    ("N=nreg-2", 102, False, 100, "mid", 3.1875),
    ("N=3", 40, False, 3, "well", 0.02),
    ("N=100-nreg=120", 120, False, 100, "well", 0.02),
    ("N=100-nreg=120", 120, False, 100, "mid", 2.25),
    ("N=255", 280, False, 255, "well", 0.02),
    ("N=255", 280, False, 255, "mid", 2.375),
    ("N=257", 280, False, 257, "well", 0.02),
    ("N=257", 280, False, 257, "mid", 2.125),
]
DUAL_LAM = 1e-10


def dual_inputs(case):
    """(y, t, f)"""
    cid, nreg, zero, N, grade, delta = case
    rng = np.random.default_rng(52000 + 3 * nreg + N + (1 if grade == "mid" else 0))
    t = np.arange(N) + delta * rng.random(N)
    f = _grid(nreg, zero, 0.3, rng)
    # a record the model explains (two coefficients of order one) with noise at 1e-6: |x| stays of order one and the bound tight, so that what an
    # unrefined alpha loses (cond u |alpha|) shows; a noise-dominated record has |x| ~ sqrt(cond) and hides it
    xt = np.zeros(nreg)
    xt[len(f) // 3], xt[len(f) // 2] = 1.0, 0.5
    y = fourier_regressor_np(t, f) @ xt + 1e-6 * rng.standard_normal(N)
    return y, t, f


def dual_cond(case):
    y, t, f = dual_inputs(case)
    A = fourier_regressor_np(t, f)
    return float(np.linalg.cond(A @ A.T + DUAL_LAM ** 2 * np.eye(len(t))))


def dual_id(case):
    return f"{case[0]}-{case[4]}-cond{dual_cond(case):.1e}"


# The refusal group: out of reach of normal equations in doubles (cond u >= 1).  (id, nreg, zero frequency, N, seed): t sorted uniform draws over
# [0, N).  The seeds are ones for which numpy's route stays below 2.5e-8 of the extended-precision solution when every entry of the regressor is
# moved by an ulp (the device's trig differs from numpy's by that much): the 1e-7 precondition holds with room on either regressor.
REFUSAL_CASES = [("fat-N64-nreg80-a", 80, False, 64, 114), ("fat-N64-nreg80-b", 80, False, 64, 145)]


def refusal_inputs(case):
    cid, nreg, zero, N, seed = case
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, N, N))
    f = _grid(nreg, zero, 0.0, rng)
    y = np.sin(2 * np.pi * f[len(f) // 3] * t) + 0.5 * rng.standard_normal(N)
    return y, t, f


def refusal_lpv_inputs():
    """ls_spectral_lpv at n > N with the default lam = 1e-8 (tests/test_gpu_regressions.py holds its fit): (Y, X, V, w, Nv)."""
    rng = np.random.default_rng(77)
    N, Nv = 60, 4
    X = np.sort(10 * rng.random(N))
    V = rng.random(N)
    w = 2 * np.pi * np.arange(1, 11) / 5.0
    Y = V * np.cos(w[2] * X) + 0.1 * rng.standard_normal(N)
    return Y, X, V, w, Nv


# ---- cases: ls_spectral_lpv ------------------------------------------------------------------------------------------------------------------
# (id, Nf, Nv, N, coulomb, normalize, progression w (-> ap), lam)
LPV_CASES = [
    ("krs-10x3", 10, 3, 400, False, True, False, 1e-3),
    ("krs-9x8", 9, 8, 400, False, True, False, 1e-3),             # n = 144: one pad strip of 112
    ("krs-8x4-coulomb", 8, 4, 400, True, True, False, 1e-3),      # nb = 2 Nv = 8, n = 128
    ("krs-10x3-raw", 10, 3, 400, False, False, False, 1e-3),      # normalize = false
    ("ap-10x3", 10, 3, 400, False, True, True, 1e-3),
]
LPV = {c[0]: c for c in LPV_CASES}


def lpv_inputs(case):
    cid, Nf, Nv, N, coulomb, normalize, prog, lam = case
    rng = np.random.default_rng(8100 + 10 * Nf + Nv + int(coulomb))
    X = rng.uniform(0.0, 20.0, N)
    V = rng.uniform(-1.0, 1.0, N)
    w = 2 * np.pi * np.arange(1, Nf + 1) / 7.0 if prog else np.sort(rng.uniform(0.4, 6.0, Nf))
    Y = (1 + V) * np.cos(w[Nf // 2] * X) + 0.3 * rng.standard_normal(N)
    return Y, X, V, w


# ---- cases: the dense estimator of the window engine -----------------------------------------------------------------------------------------
# (id, n, nwin, signals, grid, window, lam, stamp jitter, (win_lo, win_hi) or None, LPVS_NUDFT, form that must run)
# grid: "default" = default_freqs(t, n=n) (zero frequency, progression -> ap), "default-jit" = the same moved by 1e-3 of its step (no progression:
# dense), "jit0" / "jit" = non-progression with / without a zero frequency (dense).  window: rect, "hann" = Hann + 0.1, "hann0" = Hann as ls_cohere
# takes it, with which the default grid at the default lam has cond(H) ~ 1e10
WINDOW_CASES = [
    ("lone-64-rect", 64, 1, 1, "jit", "rect", 1e-3, 0.3, None, None, "dense"),
    ("two-64-hann-3sig", 64, 2, 3, "jit0", "hann", 1e-3, 0.3, None, None, "dense"),
    ("five-125-hann-2sig", 125, 5, 2, "jit", "hann", 1e-3, 0.3, None, None, "dense"),
    ("five-125-sub-1-3", 125, 5, 2, "jit0", "rect", 1e-3, 0.3, (1, 3), None, "dense"),
    ("default-lam-equidistant", 125, 5, 2, "default", "hann0", 1e-10, 0.0, None, None, "ap"),
    ("default-lam-jittered", 125, 5, 1, "default", "hann0", 1e-10, 0.3, None, None, "ap"),
    ("default-lam-jittered-direct", 125, 2, 2, "default", "hann0", 1e-10, 0.3, None, "direct", "ap"),
    ("default-lam-dense-grid", 125, 2, 1, "default-jit", "hann0", 1e-10, 0.3, None, None, "dense"),
]
WINDOWS = {c[0]: c for c in WINDOW_CASES}
# the cases that claim "problem q reads matrix q / nrhs" (equidistant stamps on the default grid give every window the same Gram: nothing to swap)
WINDOW_SWAP_CLAIMED = ("two-64-hann-3sig", "five-125-hann-2sig", "five-125-sub-1-3", "default-lam-jittered-direct")


def hann(n):
    """DSP.hanning as the library states it (symmetric, zero end points: the weighted Gram of a full default grid is singular without the ridge)."""
    return 0.5 * (1 + np.cos(2 * np.pi * np.linspace(-0.5, 0.5, n)))


def hann_plus(n):
    return hann(n) + 0.1


def window_inputs(case):
    """(Y list of signals, t, f, W or None)"""
    cid, n, nwin, ns, grid, window, lam, tj, sub, env, form = case
    rng = np.random.default_rng(9300 + n + 10 * nwin + ns + (5 if grid == "default" else 0))
    Ltot = n * nwin
    t = np.arange(Ltot) + (tj * rng.random(Ltot) if tj else 0.0)
    if grid.startswith("default"):
        fs = 1.0 / np.mean(np.diff(t[:n]))
        f = (np.arange(n // 2 + 1) * float(fs)) / n                   # default_freqs(t, n=n)
        if grid == "default-jit":
            f[1:] += 1e-3 * rng.uniform(-1, 1, len(f) - 1) * fs / n
    else:
        Nf = 24 if n == 64 else 40
        f = (np.arange(Nf) + (0.0 if grid == "jit0" else 1.0) + 0.3 * rng.uniform(-1, 1, Nf)) * (0.45 / (Nf + 1))
        if grid == "jit0":
            f[0] = 0.0
    Y = [np.sin(2 * np.pi * f[3 + 4 * q] * t + q) + 0.3 * rng.standard_normal(Ltot) + 0.2 * q for q in range(ns)]
    return Y, t, f, dict(rect=None, hann=hann_plus(n), hann0=hann(n))[window]


def window_ranges(case):
    """[(window index, slice of the record)] of the windows the case solves (noverlap = 0)."""
    n, nwin, sub = case[1], case[2], case[8]
    lo, hi = sub if sub else (0, nwin)
    return [(i, slice(i * n, (i + 1) * n)) for i in range(lo, hi)]


# ---- Sigma of ls_spectral_lpv ------------------------------------------------------------------------------------------------------------------
def var_e_bound(sys, x, Y, ones_rhs):
    """Bound on |var_e(api.py: x'Gx - 2 b'x + Y'Y and (Phi'1)'x - sum Y, in doubles, on the device's G, b) - var_e in long double|: the three dot
    products in any order (gamma_(2n), gamma_n, gamma_N <= gamma_(2n+N+4) of their absolute terms), the Gram's own entrywise error B_G, B_b (E and f
    hold them with room), and the mean's term 2 |esum| d(esum) / N."""
    n, N = sys["n"], sys["N"]
    ax = np.abs(x)
    g = gamma(2 * n + N + 4)
    absG = sys["absH"] - sys["rho"] * np.eye(n)
    e2 = g * (ax @ (absG @ ax) + 2 * np.abs(sys["b"]) @ ax + Y @ Y) + ax @ (sys["E"] @ ax) + 2 * sys["f"] @ ax
    esum = abs(float(ones_rhs @ x - Y.sum()))
    desum = g * (np.abs(ones_rhs) @ ax + np.abs(Y).sum()) + GR.bound(N, np.abs(ones_rhs)) @ ax
    return float(e2 + 2 * esum * desum / N + desum ** 2 / N) / (N - 1)


def inverse_scale(G, lam):
    """(M_ld, |M| |H| |M|) for H = G + lam I: the entrywise scale of an inverse's error (Higham, section 14: |M^ - M| <= c u |M| |H| |M| for the
    methods that are stable in this sense)."""
    M = O.inverse_ld(G, 1.0 / lam)
    aM = np.abs(M)
    return M, aM @ (np.abs(G) + lam * np.eye(G.shape[0])) @ aM


def ratio_where(err, den):
    """max |err| / den; where the scale is zero (a regressor column that is identically zero decouples) the error must be: else infinite."""
    err, den = np.abs(np.asarray(err)).astype(np.float64), np.asarray(den, dtype=np.float64)
    if np.any(err[den == 0] != 0):
        return np.inf
    return float((err[den > 0] / den[den > 0]).max())


def inverse_ratio(Mhat, M, T):
    """max |M^ - M_ld| / (u |M| |H| |M|)."""
    return ratio_where(Mhat - M, U * T)


def lpv_complex2permuted(z, Nf, nb):
    """The inverse of the LPV packing (parameter f + v Nf = c[f 2 nb + v] + i c[f 2 nb + nb + v]): the real coefficients in the device's column order."""
    z = np.asarray(z).reshape(-1)
    c = np.empty(2 * Nf * nb)
    for f in range(Nf):
        for v in range(nb):
            c[f * 2 * nb + v], c[f * 2 * nb + nb + v] = z[f + v * Nf].real, z[f + v * Nf].imag
    return c


# ---- cases: lpvs_windowpsd_lpv_f64 ---------------------------------------------------------------------------------------------------------------
WPL_N, WPL_NF, WPL_NV, WPL_LAM = 125, 8, 4, 1e-3
WPL_CASES = [(1, 1), (2, 2), (5, 1), (5, 2)]                          # (windows, in_flight)


def wpl_inputs(nwin):
    """(Y, X, V, w): nwin windows of 125 samples, a non-progression grid (the dense Gram forms)."""
    rng = np.random.default_rng(6400 + nwin)
    N = WPL_N * nwin
    X = np.sort(rng.uniform(0.0, 6.0 * nwin, N))
    V = rng.uniform(-1.0, 1.0, N)
    w = np.sort(rng.uniform(0.4, 6.0, WPL_NF))
    Y = (1 + V) * np.cos(w[3] * X) + 0.5 * np.sin(w[5] * X) + 0.2 * rng.standard_normal(N) + 0.3
    return Y, X, V, w


def wpl_window_reference(Phi, Y, lam, form="krs"):
    """One window of ls_windowpsd_lpv from the extended-precision solution: (s_f = |sum_v param|^2, its first-order bound, fva).
    With c_f = sum_v (x[f 2nb + v] + i x[f 2nb + nb + v]) and |x^ - x*| <= d componentwise (forward_bound): |c^_f - c*_f| <= D_f = the sum of d over the
    2 nb entries of frequency f, and | |c^|^2 - |c*|^2 | <= 2 |c*| D + D^2."""
    sys = system(Phi, None, Y, lam * lam, form)
    hi, lo, d = forward_bound(sys)
    x = hi.astype(LD) + lo.astype(LD)
    g = 2 * WPL_NV
    xr, dr = x.reshape(WPL_NF, g), d.reshape(WPL_NF, g)
    cre, cim = xr[:, :WPL_NV].sum(axis=1), xr[:, WPL_NV:].sum(axis=1)
    D_ = dr.sum(axis=1)
    s = cre * cre + cim * cim
    bound = 2 * np.sqrt(s.astype(np.float64)) * D_ + D_ * D_ + (g + 4) * U * s.astype(np.float64)      # + the sums and squares in doubles
    return s, bound, lpv_stats_ld(Phi, Y, x)[2]
