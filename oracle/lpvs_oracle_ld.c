/*
 * lpvs_oracle_ld.c -- the Gram-form ADMM of lpvs_oracle.c (lpvo_admm_gram: src/lasso.jl:136-171 with the
 * x-update of ProximalOperators' LeastSquares solved exactly) carried in x87 EXTENDED precision (64-bit mantissa).
 *
 * TEST INFRASTRUCTURE ONLY, like lpvs_oracle.c: an ADJUDICATOR.  When the f64 device path and the f64 oracle differ by more
 * than the stated tolerance after thousands of iterations of a map that has not converged, somebody has to say which of
 * the two is further from the iterate the reference's mathematics defines.  Same algorithm, same operation order as
 * lpvo_admm_gram (Cholesky of G + I/mu, two triangular solves per iteration, prox, dual update), every quantity --
 * factor, state vectors, prox arithmetic -- a `long double`; inputs and outputs are doubles.  2^-64 / 2^-53 = 1/2048 of the
 * double path's rounding, so at the sizes in question its iterates are exact to ~1e-12 where the f64 paths sit at ~1e-9.
 *
 * Nothing under lpvspectral.jl_amd/ links or calls this.  gcc -O2 -fopenmp (x86-64: long double = x87 80-bit).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef long double ld;

int lpvo_ld_mantissa_bits(void) { return LDBL_MANT_DIG; }

/* dot of two contiguous vectors, four independent chains (the x87 add has a 3-5 cycle latency) */
static inline ld dot_ld(const ld *a, const ld *b, int64_t n) {
    ld s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int64_t k = 0;
    for (; k + 4 <= n; k += 4) {
        s0 += a[k] * b[k]; s1 += a[k + 1] * b[k + 1]; s2 += a[k + 2] * b[k + 2]; s3 += a[k + 3] * b[k + 3];
    }
    for (; k < n; ++k) s0 += a[k] * b[k];
    return (s0 + s1) + (s2 + s3);
}

/* L row-major, lower triangle; column panels of CB so that a row's prefix is read once per CB columns */
#define CB 32
static int chol_lower_ld(ld *L, int64_t n, int verbose) {
    for (int64_t j0 = 0; j0 < n; j0 += CB) {
        const int64_t j1 = j0 + CB < n ? j0 + CB : n;
        /* the panel's own rows first (sequential in j), then every row below it in parallel */
        for (int64_t j = j0; j < j1; ++j) {
            for (int64_t c = j0; c <= j; ++c) {
                ld s = L[j * n + c] - dot_ld(L + j * n, L + c * n, c);
                if (c == j) { if (!(s > 0)) return -1; L[j * n + j] = sqrtl(s); }
                else L[j * n + c] = s / L[c * n + c];
            }
        }
#pragma omp parallel for schedule(dynamic, 8)
        for (int64_t i = j1; i < n; ++i)
            for (int64_t c = j0; c < j1; ++c)
                L[i * n + c] = (L[i * n + c] - dot_ld(L + i * n, L + c * n, c)) / L[c * n + c];
        if (verbose && (j0 / CB) % 32 == 0) { fprintf(stderr, "[ld] cholesky column %lld of %lld\n", (long long)j0, (long long)n); fflush(stderr); }
    }
    return 0;
}

/* L y = b, then L' x = y.  Row blocks of RB: the part left of (right of) the diagonal block is a mat-vec whose rows are
 * independent (threads), the diagonal block is sequential. */
#define RB 64
static void chol_solve_ld(const ld *L, const ld *Lt, int64_t n, ld *b) {
    for (int64_t i0 = 0; i0 < n; i0 += RB) {
        const int64_t i1 = i0 + RB < n ? i0 + RB : n;
#pragma omp parallel for schedule(static) if (i0 >= 1024)
        for (int64_t i = i0; i < i1; ++i) b[i] -= dot_ld(L + i * n, b, i0);
        for (int64_t i = i0; i < i1; ++i) b[i] = (b[i] - dot_ld(L + i * n + i0, b + i0, i - i0)) / L[i * n + i];
    }
    for (int64_t i1 = n; i1 > 0; i1 -= RB) {
        const int64_t i0 = i1 - RB > 0 ? i1 - RB : 0;
#pragma omp parallel for schedule(static) if (n - i1 >= 1024)
        for (int64_t i = i0; i < i1; ++i) b[i] -= dot_ld(Lt + i * n + i1, b + i1, n - i1);
        for (int64_t i = i1 - 1; i >= i0; --i) b[i] = (b[i] - dot_ld(Lt + i * n + i + 1, b + i + 1, i1 - i - 1)) / L[i * n + i];
    }
}

/* the prox operators of lpvs_oracle.c in extended precision (kinds: 1 L1, 2 L0, 3 IndBallL0, 4 group L2) */
static void prox_ld(int kind, ld *z, const ld *v, int64_t n, double param, int64_t glen, double g) {
    if (kind == 1) {
        const ld gl = (ld)g * (ld)param;
        for (int64_t i = 0; i < n; ++i) z[i] = v[i] + (v[i] <= -gl ? gl : (v[i] >= gl ? -gl : -v[i]));
    } else if (kind == 2) {
        const ld th = sqrtl(2 * (ld)g * (ld)param);
        for (int64_t i = 0; i < n; ++i) z[i] = fabsl(v[i]) > th ? v[i] : 0;
    } else if (kind == 3) {
        const int64_t r = (int64_t)param;
        if (r >= n) { memcpy(z, v, sizeof(ld) * n); return; }
        char *keep = (char *)calloc(n, 1);
        for (int64_t k = 0; k < r; ++k) {
            int64_t best = -1; ld bv = -1;
            for (int64_t i = 0; i < n; ++i) if (!keep[i] && fabsl(v[i]) > bv) { bv = fabsl(v[i]); best = i; }
            keep[best] = 1;
        }
        for (int64_t i = 0; i < n; ++i) z[i] = keep[i] ? v[i] : 0;
        free(keep);
    } else {
        for (int64_t s = 0; s + glen <= n; s += glen) {
            ld ss = 0;
            for (int64_t i = 0; i < glen; ++i) ss += v[s + i] * v[s + i];
            const ld nv = sqrtl(ss);
            ld scale = 1 - (ld)param * (ld)g / nv;
            if (!(scale > 0)) scale = 0;
            for (int64_t i = 0; i < glen; ++i) z[s + i] = scale * v[s + i];
        }
    }
}

/* G: n x n symmetric (doubles), b: n.  Runs snaps[nsnap-1] iterations from x0 (NULL: 0) with z = x0, u = 0 and writes the
 * iterates after snaps[k] iterations (ascending) to x_out / z_out / u_out [nsnap][n], rounded to double once.  No stopping test
 * (tol = 0 of the parity runs).  Returns the iterations done, or < 0. */
int64_t lpvo_admm_gram_ld(const double *G, int64_t n, const double *b, const double *x0, int prox_kind, double prox_param, int64_t glen,
                          double mu, const int64_t *snaps, int64_t nsnap, double *x_out, double *z_out, double *u_out, int verbose) {
    if (!(mu > 0 && mu <= 1) || nsnap < 1) return -2;
    ld *L = (ld *)malloc(sizeof(ld) * n * n), *Lt = (ld *)malloc(sizeof(ld) * n * n);
    ld *x = (ld *)calloc(n, sizeof(ld)), *z = (ld *)calloc(n, sizeof(ld)), *u = (ld *)calloc(n, sizeof(ld)), *t = (ld *)calloc(n, sizeof(ld));
    if (!L || !Lt || !x || !z || !u || !t) { free(L); free(Lt); free(x); free(z); free(u); free(t); return -4; }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < n; ++k) L[i * n + k] = k <= i ? (ld)G[i * n + k] + (i == k ? (ld)1 / (ld)mu : (ld)0) : (ld)0;
    if (chol_lower_ld(L, n, verbose)) { free(L); free(Lt); free(x); free(z); free(u); free(t); return -3; }
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < n; ++k) Lt[i * n + k] = k >= i ? L[k * n + i] : (ld)0;
    if (x0) for (int64_t k = 0; k < n; ++k) x[k] = z[k] = x0[k];
    int64_t it = 0, snap = 0;
    const int64_t iters = snaps[nsnap - 1];
    for (int64_t i = 1; i <= iters; ++i) {
        for (int64_t k = 0; k < n; ++k) x[k] = (ld)b[k] + (z[k] - u[k]) / (ld)mu;
        chol_solve_ld(L, Lt, n, x);
        for (int64_t k = 0; k < n; ++k) t[k] = x[k] + u[k];
        prox_ld(prox_kind, z, t, n, prox_param, glen, mu);
        for (int64_t k = 0; k < n; ++k) u[k] += x[k] - z[k];
        it = i;
        while (snap < nsnap && snaps[snap] == i) {
            for (int64_t k = 0; k < n; ++k) { x_out[snap * n + k] = (double)x[k]; z_out[snap * n + k] = (double)z[k]; u_out[snap * n + k] = (double)u[k]; }
            ++snap;
        }
        if (verbose && i % 100 == 0) { fprintf(stderr, "[ld] iteration %lld of %lld\n", (long long)i, (long long)iters); fflush(stderr); }
    }
    free(L); free(Lt); free(x); free(z); free(u); free(t);
    return it;
}

/* (G + I/mu)^-1 in extended precision, rounded to double once -> Minv_out [n][n]; b != NULL: xb = (G + I/mu)^-1 b, solved in extended
 * precision, as the double pair xb_hi + xb_lo (xb_lo may be NULL).  Returns 0, or < 0. */
int64_t lpvo_inverse_ld(const double *G, int64_t n, double mu, double *Minv_out, const double *b, double *xb_hi, double *xb_lo) {
    if (!(mu > 0) || n < 1) return -2;
    ld *L = (ld *)malloc(sizeof(ld) * n * n), *Lt = (ld *)malloc(sizeof(ld) * n * n), *t = (ld *)calloc(n, sizeof(ld));
    if (!L || !Lt || !t) { free(L); free(Lt); free(t); return -4; }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < n; ++k) L[i * n + k] = k <= i ? (ld)G[i * n + k] + (i == k ? (ld)1 / (ld)mu : (ld)0) : (ld)0;
    if (chol_lower_ld(L, n, 0)) { free(L); free(Lt); free(t); return -3; }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 0; k < n; ++k) Lt[i * n + k] = k >= i ? L[k * n + i] : (ld)0;
    for (int64_t j = 0; j < n; ++j) {
        for (int64_t k = 0; k < n; ++k) t[k] = k == j ? (ld)1 : (ld)0;
        chol_solve_ld(L, Lt, n, t);
        for (int64_t k = 0; k < n; ++k) Minv_out[k * n + j] = (double)t[k];
    }
    if (b && xb_hi) {
        for (int64_t k = 0; k < n; ++k) t[k] = (ld)b[k];
        chol_solve_ld(L, Lt, n, t);
        for (int64_t k = 0; k < n; ++k) { xb_hi[k] = (double)t[k]; if (xb_lo) xb_lo[k] = (double)(t[k] - (ld)xb_hi[k]); }
    }
    free(L); free(Lt); free(t);
    return 0;
}

/* The ADMM of lpvo_admm_gram_ld with the x-update in the offset form a device handle runs: x = xb + Mt ((z - u) / mu) for a GIVEN
 * matrix Mt [n][n] (a reduced-precision copy of the inverse, as doubles) and offset vector xb = xb_hi + xb_lo (xb_lo may be NULL);
 * every product, sum and prox in extended precision.  Same start, snapshots and return value as lpvo_admm_gram_ld. */
int64_t lpvo_admm_minv_ld(const double *Mt, int64_t n, const double *xb_hi, const double *xb_lo, const double *x0, int prox_kind, double prox_param,
                          int64_t glen, double mu, const int64_t *snaps, int64_t nsnap, double *x_out, double *z_out, double *u_out) {
    if (!(mu > 0 && mu <= 1) || nsnap < 1) return -2;
    ld *x = (ld *)calloc(n, sizeof(ld)), *z = (ld *)calloc(n, sizeof(ld)), *u = (ld *)calloc(n, sizeof(ld)), *t = (ld *)calloc(n, sizeof(ld));
    if (!x || !z || !u || !t) { free(x); free(z); free(u); free(t); return -4; }
    if (x0) for (int64_t k = 0; k < n; ++k) x[k] = z[k] = x0[k];
    int64_t it = 0, snap = 0;
    const int64_t iters = snaps[nsnap - 1];
    for (int64_t i = 1; i <= iters; ++i) {
        for (int64_t k = 0; k < n; ++k) t[k] = (z[k] - u[k]) / (ld)mu;
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < n; ++r) {
            ld s = 0;
            const double *row = Mt + r * n;
            for (int64_t k = 0; k < n; ++k) s += (ld)row[k] * t[k];
            x[r] = ((ld)xb_hi[r] + (xb_lo ? (ld)xb_lo[r] : (ld)0)) + s;
        }
        for (int64_t k = 0; k < n; ++k) t[k] = x[k] + u[k];
        prox_ld(prox_kind, z, t, n, prox_param, glen, mu);
        for (int64_t k = 0; k < n; ++k) u[k] += x[k] - z[k];
        it = i;
        while (snap < nsnap && snaps[snap] == i) {
            for (int64_t k = 0; k < n; ++k) { x_out[snap * n + k] = (double)x[k]; z_out[snap * n + k] = (double)z[k]; u_out[snap * n + k] = (double)u[k]; }
            ++snap;
        }
    }
    free(x); free(z); free(u); free(t);
    return it;
}

/* Gram of an f64 regressor in extended precision -- the reference the dense Gram kernels are held to entry by entry.
 * Phi: N x n column-major (column a contiguous), W: N row weights or NULL, Y: ns right-hand sides of N samples each ([ns][N]) or NULL.
 *   G[a][b] = sum_k W_k Phi_ka Phi_kb          S[a][b] = sum_k |W_k Phi_ka Phi_kb|          (n x n, both halves written)
 *   b[q][a] = sum_k W_k Phi_ka Y_qk            s[q][a] = sum_k |W_k Phi_ka Y_qk|            ([ns][n])
 * Every product and sum is a long double (64-bit mantissa: products of doubles round at 2^-64, integer data below 2^63 is exact);
 * each output is rounded to double once.  S and s are the scales of the a-priori bound |fl(sum) - sum| <= N u sum|terms| that holds
 * for ANY order of summation.  G or b (with their scales) may be NULL.  OpenMP over rows of G.  Returns 0, or < 0. */
int64_t lpvo_gram_ld(const double *Phi, int64_t N, int64_t n, const double *W, const double *Y, int64_t ns,
                     double *G, double *S, double *b, double *s) {
    if (N < 1 || n < 1 || !Phi || (G && !S) || (b && (!s || !Y || ns < 1))) return -2;
    int fail = 0;
#pragma omp parallel
    {
        ld *wa = (ld *)malloc(sizeof(ld) * (size_t)N);
        if (!wa) {
#pragma omp atomic write
            fail = 1;
        }
#pragma omp for schedule(dynamic, 4)
        for (int64_t ar = 0; ar < n; ++ar) {
            if (!wa) continue;
            const int64_t a = n - 1 - ar;                  /* longest rows first */
            const double *ca = Phi + a * N;
            for (int64_t k = 0; k < N; ++k) wa[k] = W ? (ld)W[k] * (ld)ca[k] : (ld)ca[k];
            for (int64_t c = 0; G && c <= a; ++c) {
                const double *cb = Phi + c * N;
                ld g0 = 0, g1 = 0, g2 = 0, g3 = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                int64_t k = 0;
                for (; k + 4 <= N; k += 4) {
                    const ld p0 = wa[k] * (ld)cb[k], p1 = wa[k + 1] * (ld)cb[k + 1], p2 = wa[k + 2] * (ld)cb[k + 2], p3 = wa[k + 3] * (ld)cb[k + 3];
                    g0 += p0; g1 += p1; g2 += p2; g3 += p3;
                    s0 += fabsl(p0); s1 += fabsl(p1); s2 += fabsl(p2); s3 += fabsl(p3);
                }
                for (; k < N; ++k) { const ld p = wa[k] * (ld)cb[k]; g0 += p; s0 += fabsl(p); }
                G[a * n + c] = G[c * n + a] = (double)((g0 + g1) + (g2 + g3));
                S[a * n + c] = S[c * n + a] = (double)((s0 + s1) + (s2 + s3));
            }
            for (int64_t q = 0; b && q < ns; ++q) {
                const double *yq = Y + q * N;
                ld g = 0, sa = 0;
                for (int64_t k = 0; k < N; ++k) { const ld p = wa[k] * (ld)yq[k]; g += p; sa += fabsl(p); }
                b[q * n + a] = (double)g;
                s[q * n + a] = (double)sa;
            }
        }
        free(wa);
    }
    return fail ? -4 : 0;
}

/* Gram of a trigonometric regressor whose PHASES w_f x_k are formed in extended precision (the structured Gram forms -- nudft.hip,
 * nufft.hip -- do not round the phase to a double as the regressor kernels do, so they are held to this one).
 *   kind 0 (LPV, permuted columns): Phi[k][f*2nb + c*nb + j] = (c ? -sin : cos)(w_f x_k) K[k][j],  K: N x nb column-major doubles
 *   kind 1 (Fourier): Phi[k][f] = cos(w_f x_k) dd, Phi[k][Nf - zf + f] = -sin(w_f x_k) dd (f >= zf), dd = 1/sqrt(2 Nf), w_f given (2 pi f
 *           as the library rounds it), zf = 1 when the first frequency is zero; K unused, nb = 1
 * G[a][b] = sum_k W_k Phi_ka Phi_kb (W NULL: 1), n x n, both halves, every quantity a long double, rounded to double once.  Returns n or < 0. */
int64_t lpvo_gram_phase_ld(int kind, const double *x, int64_t N, const double *w, int64_t Nf, const double *K, int64_t nb, int zf,
                           const double *W, double *G) {
    if (N < 1 || Nf < 1 || nb < 1 || !x || !w || !G || (kind == 0 && !K)) return -2;
    const int64_t n = kind == 0 ? 2 * Nf * nb : 2 * Nf - (zf ? 1 : 0);
    ld *Phi = (ld *)malloc(sizeof(ld) * (size_t)N * (size_t)n);      /* column-major */
    if (!Phi) return -4;
    const ld dd = 1 / sqrtl((ld)(2 * Nf));
#pragma omp parallel for schedule(static)
    for (int64_t f = 0; f < Nf; ++f)
        for (int64_t k = 0; k < N; ++k) {
            const ld ph = (ld)w[f] * (ld)x[k], c = cosl(ph), s = -sinl(ph);
            if (kind == 0) {
                for (int64_t j = 0; j < nb; ++j) {
                    Phi[(f * 2 * nb + j) * N + k] = c * (ld)K[j * N + k];
                    Phi[(f * 2 * nb + nb + j) * N + k] = s * (ld)K[j * N + k];
                }
            } else {
                Phi[f * N + k] = c * dd;
                if (!(zf && f == 0)) Phi[(Nf - (zf ? 1 : 0) + f) * N + k] = s * dd;
            }
        }
#pragma omp parallel
    {
        ld *wa = (ld *)malloc(sizeof(ld) * (size_t)N);
#pragma omp for schedule(dynamic, 4)
        for (int64_t ar = 0; ar < n; ++ar) {
            const int64_t a = n - 1 - ar;
            if (!wa) { G[a * n + a] = NAN; continue; }
            for (int64_t k = 0; k < N; ++k) wa[k] = W ? (ld)W[k] * Phi[a * N + k] : Phi[a * N + k];
            for (int64_t c = 0; c <= a; ++c) G[a * n + c] = G[c * n + a] = (double)dot_ld(wa, Phi + c * N, N);
        }
        free(wa);
    }
    free(Phi);
    return n;
}
