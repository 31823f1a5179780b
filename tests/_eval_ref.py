"""Shared by tests/test_eval_ref_host.py and tests/test_gpu_predict.py: the long-double reference of model evaluation (csrc/eval.hip),
the per-sample scale S_m its bounds are stated in, the direct path's bound, and a numpy model of the three type-2 steps.

    yhat_m[c] = s sum_f sum_j K_j(v_m) Re( p[f + j Nf, c] exp(i phi_fm) ),      S_m[c] = s sum_f sum_j |K_j(v_m)| |p[f + j Nf, c]|

The reference takes what the REFERENCE IMPLEMENTATION rounds as it rounds it -- the phase fl(w x) (Fourier: fl(fl(2 pi f) t)) and the
activation's argument fl(-gamma fl(d d)), d = fl(v - c_j), are float64 (src/lasso.jl:39, src/lsfft.jl:41, 195) -- and evaluates
everything after that (sincos, exp, the normalising sum and quotient, the products and sums) in long double.

THE DIRECT PATH'S BOUND, (Nf nb + 16) 2^-53 S_m per sample.  In units of u = 2^-53 relative to S_m, first order:
    sincos       1 ulp each = 2 u on cos and on sin;  |re| |d cos| + |im| |d sin| <= 2 u |p|                               2
    a term       t = fma(re, cos, -fl(im sin)): the product and the fma round once each, both below |p|                     2
    over f       acc += t, Nf additions in a chain, each u of a partial sum that is below the sum of the |t|            Nf - 1
    K_j          exp 1 ulp = 2 u; normalised: nb - 1 additions of non-negative terms and one quotient                   nb + 2
    over j       yhat = fma(K_j, acc_j, yhat), nb roundings                                                                nb
    s            one product; Fourier: s = 1 / sqrt(2 Nf) itself carries two roundings                                      3
which is Nf + 2 nb + 8 <= Nf nb + 10 for every nb >= 1 and Nf >= 2.  16 leaves the sincos and the exp a second ulp each (4 u) and
two units for the second-order terms, the way tests/_gram_ref.py arrives at its 16.
Against the device's own regressor times the coefficients (summed in long double) the same bound holds with room: both evaluate the
same sincos and exp on the same arguments, so those errors cancel and what remains is the arithmetic above plus one product rounding
per regressor entry.

THE TYPE-2 PATH is held to the project's structured tolerance (tests/_gram_ref.py: struct_tol) times S_m."""
import numpy as np

from _gram_ref import struct_tol  # noqa: F401  (re-exported: the GPU test takes its tolerance from here)

LD = np.longdouble
U = 2.0 ** -53
DIRECT_C = 16
TWO_PI = 6.283185307179586                       # T(2pi), src/lsfft.jl:33
PI_LD = LD("3.141592653589793238462643383279502884")
NU_W, NU_BETA = 16, 2.30 * 16                    # csrc/nufft_bins.h, csrc/nufft_coord.h
NU_MIN_GRID, NU_OVERSAMPLING, NU_MAX_GRID = 256, 3.9, 8192   # csrc/gram_form_plan.h


def direct_bound(Nf, nb, S):
    return (Nf * nb + DIRECT_C) * U * S


# ---- the activations ---------------------------------------------------------------------------------------------------------------------
def activations_ld(V, vc, gamma, normalize, coulomb):
    """K[m, j] in long double from the float64 argument the reference forms (src/lsfft.jl:195-207)."""
    V, vc = np.asarray(V, np.float64), np.asarray(vc, np.float64)
    d = V[:, None] - vc[None, :]
    arg = -gamma * (d * d)                                           # float64, rounded as written
    K = np.exp(arg.astype(LD))
    if coulomb:
        K = np.where(np.sign(V)[:, None] == np.sign(vc)[None, :], K, LD(0))
    if normalize:
        K = K / K.sum(axis=1, keepdims=True)
    return K


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def evaluate_ld(P, w, x, K=None, scale=1.0):
    """(yhat, S): long-double evaluation at the float64 phases fl(w_f x_m).  P: (Nf * nb, nc) complex in the order j Nf + f; K: (M, nb)
    long-double activations (None: one K = 1); scale: s, long double or float."""
    P = np.asarray(P, np.complex128)
    P = P.reshape(P.shape[0], -1)
    w, x = np.asarray(w, np.float64), np.asarray(x, np.float64)
    Nf, M, nc = len(w), len(x), P.shape[1]
    nb = P.shape[0] // Nf
    K = np.ones((M, 1), LD) if K is None else K
    phi = (x[:, None] * w[None, :]).astype(LD)                       # the float64 product, widened
    cs, sn = np.cos(phi), np.sin(phi)
    yh, S = np.zeros((M, nc), LD), np.zeros((M, nc), LD)
    for c in range(nc):
        for j in range(nb):
            pj = P[j * Nf:(j + 1) * Nf, c]
            re, im = pj.real.astype(LD), pj.imag.astype(LD)
            yh[:, c] += K[:, j] * (cs @ re - sn @ im)
            S[:, c] += np.abs(K[:, j]) * np.sqrt(re * re + im * im).sum()
    s = LD(scale)
    return s * yh, s * S


def fourier_scale_ld(Nf):
    return LD(1) / np.sqrt(LD(2 * Nf))


def fourier_w(f):
    return TWO_PI * np.asarray(f, np.float64)                       # fl(2 pi f), as the regressor kernel rounds it


def stack_re_im(P):
    """[re p; im p]: what the unpermuted LPV regressor multiplies."""
    P = np.asarray(P, np.complex128)
    return np.concatenate([P.real, P.imag], axis=0)


def fourier_real_vector(p, zerofreq):
    """The real coefficient vector of get_fourier_regressor's columns from the complex p (the inverse of fourier2complex)."""
    p = np.asarray(p, np.complex128)
    return np.concatenate([p.real, p.imag[1:] if zerofreq else p.imag])


# ---- a numpy model of the type-2 transform (csrc/eval.hip, steps 1-3) ------------------------------------------------------------------
def grid_size(Nf):
    nf = NU_MIN_GRID
    while nf < NU_OVERSAMPLING * Nf:
        nf *= 2
    return nf


def phihat(nf, nmodes):
    """int phi(2 t / w) cos(2 pi j t / nf) dt over the kernel's support, 96-point Gauss-Legendre in long double (csrc/nufft.hip)."""
    z, wt = np.polynomial.legendre.leggauss(96)
    z, wt = z.astype(LD), wt.astype(LD)
    half = LD(NU_W) / 2
    phi = np.exp(LD(NU_BETA) * (np.sqrt(1 - z * z) - 1))
    j = np.arange(nmodes).astype(LD)
    return (wt[None, :] * half * phi[None, :] * np.cos(2 * PI_LD * j[:, None] * (z * half)[None, :] / LD(nf))).sum(axis=1)


def progression(w):
    """a, D, eps of w_f = a + f D + eps_f as csrc/gram_form_plan.h: make_ap_slots splits it (long double)."""
    w = np.asarray(w, np.float64).astype(LD)
    a, D = w[0], (w[-1] - w[0]) / LD(len(w) - 1)
    return a, D, (w - (a + np.arange(len(w)).astype(LD) * D)).astype(np.float64)


def type2_model(p, w, x, twin=True):
    """sum_f p_f e^{i w_f x_m} by the three steps in float64 (phase reduction in long double): modes 0 .. Nf-1 of the step D on the
    fine grid, rotation by e^{i a x}, first-order twin for the residuals.  twin = False drops the twin."""
    p, x = np.asarray(p, np.complex128), np.asarray(x, np.float64)
    Nf, nf = len(p), grid_size(len(p))
    a, D, eps = progression(w)
    q = p / phihat(nf, Nf).astype(np.float64)
    k, f = np.arange(nf), np.arange(Nf)
    ang = 2 * PI_LD * (np.arange(nf).astype(LD) / nf)
    tw = np.cos(ang).astype(np.float64) + 1j * np.sin(ang).astype(np.float64)       # exact table, indexed by f k mod nf
    qs = [q] + ([1j * eps * q] if twin and np.any(eps != 0) else [])
    grids = [np.zeros(nf, np.complex128) for _ in qs]
    for f0 in range(0, Nf, 128):                                     # (chunks of frequencies: the 2100 x 8192 table is never whole)
        Ec = tw[(f[f0:f0 + 128, None] * k[None, :]) % nf]
        for g, qq in zip(grids, qs):
            g += qq[f0:f0 + 128] @ Ec
    turns = (D * x.astype(LD)) / (2 * PI_LD)
    r = turns - np.floor(turns)
    pos = (r * nf).astype(np.float64)
    pos = np.where(pos >= nf, pos - nf, pos)
    g0 = np.ceil(pos - NU_W / 2).astype(np.int64)
    out = np.zeros(len(x), np.complex128)
    for gi, g in enumerate(grids):
        acc = np.zeros(len(x), np.complex128)
        for kk in range(NU_W):
            z = ((g0 + kk) - pos) * (2.0 / NU_W)
            s = 1.0 - z * z
            tap = np.where(s > 0, np.exp(NU_BETA * (np.sqrt(np.maximum(s, 0.0)) - 1.0)), np.exp(-NU_BETA))
            acc += tap * g[(g0 + kk) % nf]
        out += acc if gi == 0 else x * acc
    ta = (a * x.astype(LD)) / (2 * PI_LD)
    ta = 2 * PI_LD * (ta - np.floor(ta))
    rot = np.cos(ta).astype(np.float64) + 1j * np.sin(ta).astype(np.float64)
    return rot * out
