/*
 * lpvspectral.h -- C-ABI of the MI355X-native regression-matrix + ADMM hot path of
 * LPVSpectral.jl.  This is the drop-in boundary: a Julia wrapper keeps the reference's
 * function signatures and reaches these entry points through @ccall;
 * the Python host mirror in lpvspectral.jl_amd/ reaches them through ctypes.
 *
 * Conventions
 *   - every function returns an int32 status (LPVS_OK or a negative LPVS_E* code);
 *     lpvs_last_error() gives the thread-local message of the last failure.
 *   - sizes are int64_t (Julia Int); matrices are COLUMN-MAJOR (Julia layout).
 *   - every floating-point array argument may be a HOST pointer or a DEVICE (HIP) pointer of the
 *     current device; the library detects which (hipPointerGetAttributes).  Integer outputs
 *     (int64_t* counts, offsets, iteration counts) and scalar outputs are HOST pointers.  The
 *     caller owns all argument memory; it is never retained or freed here, and is
 *     only read/written for the duration of the call.  Device arguments are read on the
 *     library's own streams: work the caller has queued on other streams to produce them
 *     must be complete before the call (the Python mirror synchronises torch's current
 *     stream; a Julia wrapper calls AMDGPU.synchronize()).  Device outputs are complete
 *     when the call returns.
 *   - a handle owns one HIP stream on one device; handles are not thread-safe,
 *     different handles may be used concurrently.
 *   - arithmetic type: fp64 (suffix _f64), the eltype of every reference test: assembly, Gram,
 *     factorisation, prox operators and every accumulation are double.  STORAGE CAVEAT: for
 *     n >= 2048 the ADMM mat-vec of an _f64 handle streams, by default, a reduced-width COPY of
 *     (G + I/mu)^-1 with >= 36 significant bits per element (LPVS_STORAGE_MIXED below), applied in
 *     offset form x = M b + M~ (z-u)/mu with M b from the full doubles.  Measured cost: 1.1e-10
 *     rel-L2 in z after 2000 iterations at N = 2^20, n = 8192 -- below the reference's own CG
 *     tolerance sqrt(eps) = 1.5e-8 (src/lasso.jl:151, ProximalOperators iterative=true).
 *     lpvs_problem_set_option(h, LPVS_OPT_M_STORAGE, LPVS_STORAGE_F64) streams the doubles
 *     themselves (1.55x the bytes per iteration).
 *
 * File:line citations are into the reference (baggepinnen/LPVSpectral.jl v0.3.4).
 */
#ifndef LPVSPECTRAL_H
#define LPVSPECTRAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPVS_VERSION 100 /* 0.1.0 */

/* status codes -> exception the Julia/Python wrapper raises */
#define LPVS_OK 0
#define LPVS_EARGUMENT (-1)    /* ArgumentError: zero frequency not first        src/lsfft.jl:22   */
#define LPVS_EASSERT (-2)      /* AssertionError: mu outside [0,1], length mismatch src/lasso.jl:143, src/windows.jl:31 */
#define LPVS_EDOMAIN (-3)      /* DomainError: noverlap >= n (DSP.arraysplit)    src/windows.jl:33 */
#define LPVS_ENOMEM (-4)       /* host or device allocation failed */
#define LPVS_EDEVICE (-5)      /* HIP runtime error / no gfx950 device */
#define LPVS_EUNSUPPORTED (-6) /* e.g. coulomb=true in the sparse LPV path (note ++) */
#define LPVS_ENUMERIC (-7)     /* (G + I/mu) not positive definite */
#define LPVS_ESTATE (-8)       /* call order violated (run before init, ...) */

/* prox_g kinds (ProximalOperators.jl objects at src/lasso.jl:53-55,88,108; README.md:70-83) */
#define LPVS_PROX_L1 1       /* NormL1(lam):  soft threshold at mu*lam */
#define LPVS_PROX_L0 2       /* NormL0(lam):  keep |v| > sqrt(2*mu*lam) */
#define LPVS_PROX_BALL_L0 3  /* IndBallL0(r): keep the r largest |v| (param = r) */
#define LPVS_PROX_GROUP_L2 4 /* SlicedSeparableSum(NormL2(lam)) on contiguous groups of group_len */

/* linear-term convention of the x-update, lpvs_admm_init(..., linear_sign) */
#define LPVS_LINEAR_LEAST_SQUARES (+1) /* LeastSquares(A,y): (G+I/mu)x =  b + v/mu   src/lasso.jl:51,98 */
#define LPVS_LINEAR_QUADRATIC_AS_WRITTEN (-1) /* Quadratic(Q,q=+A'Wy): (Q+I/mu)x = -q + v/mu   src/lasso.jl:119-121 */

typedef struct lpvs_problem lpvs_problem;

/* ---- library ------------------------------------------------------------------------ */
int32_t lpvs_version(void);
int32_t lpvs_device_count(void);          /* number of visible HIP devices (0 if none) */
const char *lpvs_last_error(void);        /* thread-local, valid until the next failing call */
/* work buffers are cached per device between calls (cap: LPVS_POOL_GIB, default 128); this returns them to the driver */
int32_t lpvs_release_cached_memory(void);

/* ---- options: how a handle stores the inverse its ADMM mat-vec streams, how it iterates, which Gram form its constructor
 * takes.  Value 0 (LPVS_OPT_DEFAULT) = the library's choice, which an environment variable of the same name may override for
 * experiments (LPVS_M_STORAGE, LPVS_ITERATION, LPVS_GRAM_FORM, LPVS_NT_LOADS, LPVS_NUDFT, LPVS_WINDOW_CHUNK_MB [0 = uncut],
 * LPVS_WINDOWS_IN_FLIGHT, LPVS_RESERVE_CUS [0 = none]); an explicit option wins over the
 * environment.  Results do not depend on ITERATION / NT_LOADS / SLOT_SUMS beyond rounding (tests/test_gpu_one_launch.py,
 * tests/test_gpu_nufft.py); M_STORAGE trades bytes per iteration against 1e-10 in the iterates (see the header comment).
 *   lpvs_set_default_option:  thread-local default for handles created and batched-window calls made AFTERWARDS by the calling
 *                             thread (the batched-window entry points have no handle to carry options);
 *   lpvs_problem_set_option:  one handle.  ITERATION / NT_LOADS take effect at the next lpvs_admm_run; a CHANGED M_STORAGE
 *                             invalidates the iteration state (the packed copy is rebuilt): lpvs_admm_init must follow, an
 *                             lpvs_admm_run without it returns LPVS_ESTATE;
 *                             GRAM_FORM and SLOT_SUMS are constructor-time choices, WINDOW_CHUNK_MB / WINDOWS_IN_FLIGHT / RESERVE_CUS
 *                             belong to calls without a handle or to the device (LPVS_ESTATE on a handle: set the default). */
#define LPVS_OPT_DEFAULT 0
#define LPVS_OPT_M_STORAGE 1  /* LPVS_STORAGE_*  : packed inverse of n >= 2048 handles / window batches */
#define LPVS_OPT_ITERATION 2  /* LPVS_ITERATION_*: one launch per ADMM iteration (where applicable) or mat-vec + update launches */
#define LPVS_OPT_GRAM_FORM 3  /* LPVS_GRAM_*     : structured Gram for arithmetic-progression grids, or the dense MFMA forms */
#define LPVS_OPT_NT_LOADS 4   /* LPVS_NT_*       : non-temporal tile loads (default: when a launch streams more than 240 MiB of inverses -- window batches, single problems from n = 10752) */
#define LPVS_OPT_SLOT_SUMS 5  /* LPVS_SLOTS_*    : slot sums of the structured Gram by non-uniform FFT or by direct evaluation */
#define LPVS_STORAGE_MIXED 1  /* float head + 16-bit tail (40 bits) for tiles with large entries, 36-bit fixed point elsewhere, all 36 bits read by every iteration */
#define LPVS_STORAGE_SPLIT 2  /* float head + 16-bit tail everywhere (6 bytes, 40 significant bits) */
#define LPVS_STORAGE_F64 3    /* doubles (8 bytes): the reference-width copy */
#define LPVS_STORAGE_MIXED32 4 /* MIXED, but the iteration READS the 32 leading bits of the fixed-point tiles only (4 B per element: 140 instead of 157 MB per
                                * iteration at n = 8192) and the product of the 4-bit planes is taken with a right-hand side at most 32 iterations old (1, 2, 4, ... in the first 256), carried
                                * in the x-update's offset vector ("stale nibble product").  THE DEFAULT of handles whose x-update is
                                * corrected (one right-hand side, doubles, n >= 2048 -- LPVS_OPT_XUPDATE_CORRECTION); MIXED for every other handle, also when
                                * asked for by name.  x, z and u stay where MIXED leaves them: at cfg3 after 200 .. 2000 iterations x and z are the same
                                * 1.2e-10 .. 4.8e-10 from the exact iterates and u 9.8e-11 .. 5.0e-10 (MIXED: 9.6e-11 .. 4.5e-10) --
                                * profiles/r05_cfg3_stale_nibble_product.txt.  (Without the refresh the dual variable integrates the truncation: u 2e-9 .. 7e-9.) */
#define LPVS_ITERATION_ONE 1
#define LPVS_ITERATION_TWO 2
#define LPVS_GRAM_AP 1        /* structured (error unless the grid is an arithmetic progression up to rounding) */
#define LPVS_GRAM_KRS 2       /* dense, symmetric-pair contraction */
#define LPVS_GRAM_KR 3        /* dense, Khatri-Rao contraction */
#define LPVS_NT_OFF 1
#define LPVS_NT_ON 2
#define LPVS_OPT_WINDOW_CHUNK_MB 6   /* batched-window engine: MB (10^6 bytes) of packed inverses per chunk (a chunk is re-read from the Infinity
                                       * Cache every iteration); > 0: that many MB, LPVS_WINDOW_UNCUT: every window in one launch per iteration;
                                       * default: 1.0625 x the Infinity Cache of the GPU nodes of the KFD topology (256 MiB on MI355X = 268.4 MB
                                       * -> 285 MB) */
#define LPVS_OPT_WINDOWS_IN_FLIGHT 7 /* parts of a chunk solved concurrently on streams of their own: 1 .. 4 (default 2) */
#define LPVS_OPT_RESERVE_CUS 8       /* CUs the factorisation's trailing updates leave to its pivot chain: > 0, or LPVS_RESERVE_NONE (default 8) */
#define LPVS_OPT_XUPDATE_CORRECTION 9 /* LPVS_XCORR_*: re-form the x-update's offset vector after the iterations 16, 128, 256, 512, 1024, ... (several right-hand sides: 16, 512, 1024, ...) by one step of iterative
                                       * refinement, residual accumulated in twice the mantissa (handles of n >= 2048).  Default: ON -- since
                                       * round 6 also for handles with several right-hand sides (cfg5: 4e-10 of drift in x, z after 2000 iterations without it;
                                       * a correction there is one accurate pass over the f64 Gram for all channels, 1.9 % of the run).  Per handle (before
                                       * lpvs_admm_init) or as a thread default. */
#define LPVS_XCORR_ON 1
#define LPVS_XCORR_OFF 2
#define LPVS_SLOTS_NUFFT 1
#define LPVS_SLOTS_DIRECT 2
#define LPVS_WINDOW_UNCUT (-1)
#define LPVS_RESERVE_NONE (-1)
int32_t lpvs_set_default_option(int32_t option, int32_t value);
int32_t lpvs_get_default_option(int32_t option, int32_t *value);   /* the calling thread's explicit default (0 if none) */
int32_t lpvs_problem_set_option(lpvs_problem *h, int32_t option, int32_t value);
int32_t lpvs_problem_get_option(lpvs_problem *h, int32_t option, int32_t *value);   /* the value in effect for this handle */

/* ---- a1  check_freq                                                  src/lsfft.jl:20-24
 * *zerofreq = 0 (no zero frequency) or 1 (zero frequency is first); LPVS_EARGUMENT if a
 * zero frequency sits elsewhere.  Host pointers only (tiny). */
int32_t lpvs_check_freq_f64(const double *f, int64_t Nf, int64_t *zerofreq);

/* ---- a2  get_fourier_regressor(t,f)                                  src/lsfft.jl:26-49
 * A_out is N x Nreg column-major, Nreg = 2Nf - (zerofreq ? 1 : 0):
 *   A[n,k] = cos((2pi f_k) t_n)/sqrt(2Nf);  A[n,k+sinoffset] = -sin(...)/sqrt(2Nf). */
int32_t lpvs_fourier_regressor_f64(const double *t, int64_t N, const double *f, int64_t Nf,
                                   double *A_out, int64_t *zerofreq);

/* ---- a3  basis_activation_func evaluated on all samples   src/utilities.jl:23-36, src/lsfft.jl:195-207
 * K_out is N x nb column-major, nb = Nv (2Nv if coulomb). */
int32_t lpvs_basis_activation_f64(const double *V, int64_t N, int64_t Nv, int32_t normalize,
                                  int32_t coulomb, double *K_out);

/* ---- a4+a5  LPV regressor                          src/lasso.jl:35-50, src/lsfft.jl:240-247
 * permuted != 0: Phi = [Re As, Im As][:, inds]  (N x 2*Nf*nb, each frequency's 2nb columns
 * adjacent, the matrix ls_sparse_spectral_lpv solves on); permuted == 0: [Re As, Im As]. */
int32_t lpvs_lpv_regressor_f64(const double *X, const double *V, int64_t N, const double *w,
                               int64_t Nf, int64_t Nv, int32_t normalize, int32_t coulomb,
                               int32_t permuted, double *Phi_out);

/* ---- problem handles: regressor assembly + Gram on device ----------------------------
 * Each constructor builds G (n x n) and b (n) on `device` and keeps them resident:
 *   fourier: G = A' diag(W) A, b = A' diag(W) y  (W == NULL: identity)  src/lasso.jl:91,98 / :111,118-120
 *   lpv:     G = Phi' Phi,     b = Phi' y   (Phi never materialised)    src/lasso.jl:35-51
 *   gram:    G, b supplied by the caller (any Quadratic(Q,q) / LeastSquares in Gram form).
 *   dense:   see below. */
int32_t lpvs_problem_create_fourier_f64(const double *y, const double *t, int64_t N, const double *f,
                                        int64_t Nf, const double *W, int32_t device,
                                        lpvs_problem **out);
int32_t lpvs_problem_create_lpv_f64(const double *y, const double *X, const double *V, int64_t N,
                                    const double *w, int64_t Nf, int64_t Nv, int32_t normalize,
                                    int32_t coulomb, int32_t device, lpvs_problem **out);
/* lpv_multi: ns signals sharing (X, V, w) -- Y is N x ns column-major (multichannel records): ONE Gram, ns
 *          right-hand sides b_q = Phi' y_q; every ADMM kernel then advances all ns signals in one pass over M,
 *          each with its own convergence flag and iteration count (extension: the reference has no batched
 *          entry point, SURVEY.md section 8(b) "Gaps").  x0 / iterates / params are n x ns (resp. m x ns). */
int32_t lpvs_problem_create_lpv_multi_f64(const double *Y, int64_t ns, const double *X, const double *V, int64_t N,
                                          const double *w, int64_t Nf, int64_t Nv, int32_t normalize,
                                          int32_t coulomb, int32_t device, lpvs_problem **out);

/* ---- one exchange step for a single large problem: the sample rows of one signal are sharded
 * across devices, every shard forms its partial Gram G_r = Phi_r' Phi_r and b_r = Phi_r' y_r, the partials are
 * summed (RCCL all-reduce on the device pointers below) and the ADMM runs replicated.  The basis centres of
 * src/utilities.jl:24-32 depend on min/max of V over ALL rows, so a shard is built with the global ranges:
 *   ranges4 = {min V, max V, max|V|, max|X|}   (lpvs_lpv_ranges_f64 gives a shard's own; combine with min/max)
 * max|X| only steers the choice of Gram form, which must be the same on every shard. */
int32_t lpvs_lpv_ranges_f64(const double *X, const double *V, int64_t N, double *out4);

/* ---- model evaluation (extension: the reference has no predict): the fitted model at M samples without the regressor,
 *   yhat_m[c] = s sum_f sum_j K_j(v_m) Re( p[f + j Nf, c] exp(i phi_fm) )
 * Fourier: s = 1/sqrt(2 Nf), one K = 1, phi = (2 pi f_f) t_m, p = what lpvs_ls_spectral_f64 returns -- the result is the regressor of
 * lpvs_fourier_regressor_f64 times the coefficients.  LPV: s = 1, phi = w_f x_m, p in the reference's order j Nf + f
 * (lpvs_problem_get_params_f64), K the activations with centres built from ranges3 = {min V, max V, max|V|} of the TRAINING record
 * (lpvs_lpv_ranges_f64), so that new samples meet the fitted basis -- the regressor of lpvs_lpv_regressor_f64 (permuted = 0) times
 * [re p; im p].  nc coefficient columns (a regularisation path) are evaluated in one call, each to the bits of its own call.
 * path: 0 auto, 1 direct sums (any grid), 2 type-2 non-uniform FFT (grids that are an arithmetic progression up to rounding, within
 * the fine-grid limit: LPVS_EARGUMENT otherwise).  y may be NULL: out = yhat, else out = y - yhat; out is M x nc column-major.
 * sums (host, 2 nc doubles, may be NULL): sum and sum of squares of every output column, in a fixed order (two calls, same bits).
 * t / X / V / y / out: host or device memory; coefficients, f / w and ranges3: host memory.
 * lpvs_eval_last_timing (the calling thread's last call): [0] path taken, [1] fine grid size (0: direct), [2] the first-order twin
 * grids ran, ms of [3] staging and the reduction of max|x|, [4] the fine grids, [5] the interpolation or the direct sums, [6] the
 * sums, [7] the copy-out, [8] total, [9] slabs of partial sums per column. */
int32_t lpvs_fourier_eval_f64(const double *p_re, const double *p_im, int64_t nc, const double *f, int64_t Nf,
                              const double *t, const double *y, int64_t M, int32_t path, int32_t device,
                              double *out, double *sums);
int32_t lpvs_lpv_eval_f64(const double *p_re, const double *p_im, int64_t nc, const double *w, int64_t Nf, int64_t Nv,
                          int32_t normalize, int32_t coulomb, const double *ranges3,
                          const double *X, const double *V, const double *y, int64_t M, int32_t path, int32_t device,
                          double *out, double *sums);
int32_t lpvs_eval_last_timing(double *out, int32_t n);
int32_t lpvs_problem_create_lpv_rows_f64(const double *Y, int64_t ns, const double *X, const double *V,
                                         int64_t N_local, const double *w, int64_t Nf, int64_t Nv,
                                         int32_t normalize, int32_t coulomb, const double *ranges4,
                                         int32_t device, lpvs_problem **out);
/* device pointers of the handle's Gram (np x np, leading dimension np, full symmetric storage, pad rows and
 * columns zero) and right-hand sides (np per signal); valid while the handle lives.  After modifying them in
 * place call lpvs_problem_gram_modified so that the cached factorisation is dropped. */
int32_t lpvs_problem_device_gram_f64(lpvs_problem *h, double **G_dev, double **b_dev, int64_t *np);
int32_t lpvs_problem_gram_modified(lpvs_problem *h);
int32_t lpvs_problem_num_signals(const lpvs_problem *h, int64_t *ns);
/* dense:   A (m x n column-major) supplied by the caller: G = A' diag(W) A, b = A' diag(W) y --
 *          the generic ADMM(x, LeastSquares(A,y,iterative=true), proxg) plugin path, src/lasso.jl:136 */
int32_t lpvs_problem_create_dense_f64(const double *A, const double *y, int64_t m, int64_t n,
                                      const double *W, int32_t device, lpvs_problem **out);
int32_t lpvs_problem_create_gram_f64(const double *G, const double *b, int64_t n, int32_t device,
                                     lpvs_problem **out);
/* path:    a new handle with ns right-hand sides from a single-signal handle of ANY constructor above (LPVS_EARGUMENT if src has
 *          several signals, or unless 1 <= ns <= 64): src's kind, sizes, zerofreq, parameter packing, _f32 flag and options; its Gram
 *          is a device-to-device copy of src's and each of its ns right-hand sides is src's b.  src stays valid and independent (it
 *          may be destroyed first).  With lpvs_problem_set_prox_per_signal: ns penalties solved in one pass over one inverse. */
int32_t lpvs_problem_create_path(lpvs_problem *src, int64_t ns, lpvs_problem **out);
int32_t lpvs_problem_destroy(lpvs_problem *h);

int32_t lpvs_problem_size(const lpvs_problem *h, int64_t *n);
int32_t lpvs_problem_zerofreq(const lpvs_problem *h, int64_t *zerofreq);
/* copy out G (n x n, full symmetric) and/or b (n); either pointer may be NULL */
int32_t lpvs_problem_get_gram_f64(lpvs_problem *h, double *G_out, double *b_out);

/* all right-hand sides b_q = Phi' y_q of a (multi-signal) handle, n x ns column-major */
int32_t lpvs_problem_get_rhs_f64(lpvs_problem *h, double *b_out);
/* (G + shift*I)^-1 (n x n, symmetric) -- e.g. the parameter covariance of ls_spectral_lpv up to the factor var(e),
 * src/lsfft.jl:252-254.  Leaves the handle's factorisation cached for that shift. */
int32_t lpvs_problem_get_inverse_f64(lpvs_problem *h, double shift, double *Minv_out);
/* The same after one round of iterative refinement against G + shift*I (column q: x += M (e_q - (G + shift*I) x)): an inverse that is itself the
 * result -- the covariance above -- at the accuracy of a pivoted factorisation whatever the number of 128-blocks the sweep eliminates by;
 * symmetric up to rounding, column q in Minv_out[q*n .. q*n + n).  Four n x n work arrays on the device. */
int32_t lpvs_problem_get_inverse_refined_f64(lpvs_problem *h, double shift, double *Minv_out);

/* ---- dense (ridge) solve from the same Gram:  (G + ridge*I) x = b ---------------------
 * ls_spectral weighted form (src/lsfft.jl:77, ridge = lam), fourier_solve / real_complex_bs in
 * normal-equation form (src/utilities.jl:49-60, ridge = lam^2).  x_out has n entries in the
 * regressor's column order. */
int32_t lpvs_problem_solve_ridge_f64(lpvs_problem *h, double ridge, double *x_out);

/* ---- ls_spectral(y,t,f; lam): [A; lam I] \ [y; 0]                src/lsfft.jl:62-67, src/utilities.jl:56-60
 * The minimiser is computed from a Gram on device, in the better-conditioned of its two forms:
 *   N >= Nreg (tall):  x = (A'A + lam^2 I)^-1 A'y          (primal normal equations)
 *   N <  Nreg (fat):   x = A' (A A' + lam^2 I)^-1 y        (dual form; e.g. default_freqs of an even-length t
 *                                                           has Nreg = N+1 and a vanishing Nyquist sine column)
 * Either solve is the explicit inverse refined twice against its own system; LPVS_ENUMERIC when that system is singular to working
 * precision (a non-positive pivot, or a relative residual above 1e-9 after the refinement): the bindings then solve [A; lam I] by QR on the host.
 * re/im: Nf entries, fourier2complex of x. */
int32_t lpvs_ls_spectral_f64(const double *y, const double *t, int64_t N, const double *f, int64_t Nf, double lam,
                             int32_t device, double *re_out, double *im_out);

/* ---- ADMM                                                          src/lasso.jl:136-171
 * set_prox: the g of z <- prox_{mu g}(x+u).  init: x <- x0 (zeros if NULL), z <- x, u <- 0,
 * factorises (G + I/mu) once (LPVS_EASSERT unless 0 <= mu <= 1).  run: up to max_iters more
 * iterations, stopping after the first with ||x-z||_2 < tol exactly as src/lasso.jl:164; it
 * returns to the caller so that printing, cb(x,z) and Ctrl-C stay on the host thread
 * (src/lasso.jl:158-163, :59-63).  *iters_done counts iterations since init. */
int32_t lpvs_problem_set_prox(lpvs_problem *h, int32_t kind, double param, int64_t group_len);
/* one prox parameter per signal slot of a handle with several right-hand sides (extension: a regularisation path, or one penalty per
 * channel): params[q] is the lambda -- or the r of LPVS_PROX_BALL_L0 -- of signal q; kind and group_len are shared.  count must be the
 * handle's number of signals (LPVS_EARGUMENT otherwise, as for a negative or non-finite parameter); params may live on the host or on a
 * device and is copied.  Checks and invalidates what lpvs_problem_set_prox does; a later lpvs_problem_set_prox returns the handle to
 * one parameter for all.  Nothing but the prox reads the parameter: Gram, inverse, packing, offset vector and correction schedule are
 * shared, every signal keeps its own iteration count and stopping test, and signal q's iterates are those of a handle whose
 * lpvs_problem_set_prox was given params[q]. */
int32_t lpvs_problem_set_prox_per_signal(lpvs_problem *h, int32_t kind, const double *params, int64_t count, int64_t group_len);
/* the parameter every signal's prox will read (count = the handle's number of signals): the scalar repeated when no per-signal values
 * are installed.  out may live on the host or on a device. */
int32_t lpvs_problem_get_prox_params(lpvs_problem *h, double *out, int64_t count);
int32_t lpvs_admm_init_f64(lpvs_problem *h, const double *x0, double mu, double tol,
                           int32_t linear_sign);
int32_t lpvs_admm_run(lpvs_problem *h, int64_t max_iters, int64_t *iters_done, double *nxz,
                      int32_t *converged);
/* resume (checkpoint / re-entry): after lpvs_admm_init (same mu, tol, prox, linear_sign) install iterates
 * saved with lpvs_admm_get_f64 from an earlier run -- possibly of another process -- together with the number of
 * iterations they represent; lpvs_admm_run then continues as the uninterrupted run would (the x-update of src/lasso.jl:150-151 only
 * needs z and u) -- BIT FOR BIT for handles of n < 2048; handles of n >= 2048 also carry the x-update's offset vector between two
 * scheduled iterations (below): with it (lpvs_admm_set_offset_f64) the continuation is bit-exact, without it the vector is re-formed from
 * the state handed in and the continuation agrees to second order (~1e-12).  iters_done = 0 restarts: the offset vector of a fresh
 * lpvs_admm_init is put back.  Arrays are n (x ns) in the solver's own order, as lpvs_admm_get_f64 returns. */
int32_t lpvs_admm_set_state_f64(lpvs_problem *h, const double *x, const double *z, const double *u, int64_t iters_done);
/* Handles of n >= 2048 run the x-update in its offset form, x = xb + M (z - u)/mu, and re-form the offset vector after the iterations
 * 16, 128, 256, 512, 1024, ... (handles with several right-hand sides: 16, 512, 1024, ...) so that the systematic error of the explicit inverse leaves the iteration (one step of iterative refinement
 * with the residual accumulated in twice the mantissa).  That vector is part of the iteration's state between two
 * scheduled iterations: a checkpoint that is to continue BIT FOR BIT saves it with lpvs_admm_get_offset_f64 next to x, z, u and
 * installs it with lpvs_admm_set_offset_f64 after lpvs_admm_set_state_f64 (which, without it, re-forms the vector from the state it is
 * given -- the same to second order).  Always doubles (also for handles made by the _f32 constructors).
 * lpvs_admm_offset_len: how many -- n x ns, or 2 n for a handle that iterates on LPVS_STORAGE_MIXED32 reads (the vector with and without
 * the nibble term of the last refresh: both are state); 0 when the handle has no offset vector (n < 2048).  The buffer is opaque: hand
 * back what lpvs_admm_get_offset_f64 wrote.  `len` = the number of doubles the caller's buffer holds and must EQUAL lpvs_admm_offset_len
 * (LPVS_EARGUMENT otherwise: a checkpoint written by a 36-bit handle does not go into a handle that reads 32 bits, or the reverse -- nothing
 * is read or written past a buffer of the wrong size).  get / set: LPVS_ESTATE when the handle has no offset vector, or before lpvs_admm_init. */
int32_t lpvs_admm_offset_len(lpvs_problem *h, int64_t *len);
int32_t lpvs_admm_get_offset_f64(lpvs_problem *h, double *xb_out, int64_t len);
int32_t lpvs_admm_set_offset_f64(lpvs_problem *h, const double *xb, int64_t len);
/* per-signal state of a multi-signal handle (lpvs_admm_run reports the slowest signal / the largest ||x-z||) */
int32_t lpvs_admm_status(lpvs_problem *h, int64_t signal, int64_t *iters_done, double *nxz, int32_t *converged);
/* iterates in the solver's own (regressor-column) order; any pointer may be NULL */
int32_t lpvs_admm_get_f64(lpvs_problem *h, double *x_out, double *z_out, double *u_out);

/* ---- a14 result packing ---------------------------------------------------------------
 * fourier: fourier2complex(z, zerofreq)                         src/utilities.jl:62-73
 * lpv:     z[sortperm(inds)] -> complex, index f+(v-1)Nf        src/lasso.jl:67-68
 * which = 0: pack z (what the estimators return), 1: pack x.  re/im have Nf (fourier) or
 * Nf*nb (lpv) entries. */
int32_t lpvs_problem_get_params_f64(lpvs_problem *h, int32_t which, double *re_out, double *im_out);
/* same packing applied to a caller-supplied coefficient vector (e.g. a ridge solution) */
int32_t lpvs_problem_pack_params_f64(lpvs_problem *h, const double *coef, double *re_out,
                                     double *im_out);

/* ---- timing: HIP-event durations (ms) of the handle's phases, measured on its stream ---
 * out[0] basis tables, out[1] Gram kernel(s), out[2] Gram reduce + rhs, out[3] factorisation,
 * out[4] ADMM iterations (sum over lpvs_admm_run calls), out[5] flops the Gram kernel's MFMA core
 * actually issues (tiles*128*256*2*Npad; the structured form: 8*N*(3Nf-1)*P VALU flops), out[6]
 * algorithmic Gram flops N*n*(n+1), out[7] ADMM iterations timed in out[4], out[8] Gram form used:
 * 0 none (Gram given), 1 n x n lower triangle, 2 symmetric-pair, 3 k-major panel, 4 structured
 * (arithmetic-progression w, nudft.hip), 5 structured with the slot sums by non-uniform FFT; out[9] the time of the x-update
 * corrections inside out[4] (HIP events around each), out[10] their count; out[11] the refreshes of the stale nibble product
 * enqueued inside out[4] (LPVS_STORAGE_MIXED32), out[12] the duration of one (us) where a refresh is three kernels of its own (the two-launch
 * iteration; measured stand-alone by lpvs_admm_time_matvec) -- 0 before that call and for the one-launch iteration, whose refresh is part
 * of the launch it follows (that launch also multiplies the 4-bit planes) plus one vector kernel; out[13] the samples per stage of the
 * dense Gram kernel instance that was launched (gram_kernel<MODE, BK>: 32, 16 or 8) and out[14] the number of sample chunks its tiles were
 * split into -- both 0 for a given or structured Gram.  n_out values are written (at most 15): a caller asking for 13 gets the first 13. */
int32_t lpvs_problem_get_timing(lpvs_problem *h, double *out, int32_t n_out);

/* average duration (microseconds) of the ADMM mat-vec kernel of this handle over `reps` back-to-back launches, from
 * HIP events on the handle's stream (benchmark instrumentation; needs lpvs_admm_init; iterates are not modified).
 * *bytes_per_launch = bytes of M the kernel streams per launch (tile-packed lower triangle, or the full matrix). */
int32_t lpvs_admm_time_matvec(lpvs_problem *h, int32_t reps, double *us_per_launch, double *bytes_per_launch);

/* ---- single-precision entry points ------------------------------------------------------
 * The reference is eltype-generic (src/lasso.jl:85,91,144: Float32 inputs run in Float32).  The
 * _f32 functions take and return float arrays (host or device).  Inputs are widened exactly to
 * double; assembly, Gram and factorisation run in double (at least as accurate as a Float32 run
 * of the reference); a handle created here streams a single-precision copy of (G + I/mu)^-1 in
 * the ADMM mat-vec of large problems (half the bytes per iteration, double accumulation);
 * outputs are rounded to float.  Handle functions without a type suffix (set_prox, admm_run,
 * admm_status, timing, destroy, ...) are shared with the _f64 handles. */
int32_t lpvs_check_freq_f32(const float *f, int64_t Nf, int64_t *zerofreq);
int32_t lpvs_fourier_regressor_f32(const float *t, int64_t N, const float *f, int64_t Nf,
                                   float *A_out, int64_t *zerofreq);
int32_t lpvs_lpv_regressor_f32(const float *X, const float *V, int64_t N, const float *w, int64_t Nf,
                               int64_t Nv, int32_t normalize, int32_t coulomb, int32_t permuted,
                               float *Phi_out);
int32_t lpvs_problem_create_fourier_f32(const float *y, const float *t, int64_t N, const float *f,
                                        int64_t Nf, const float *W, int32_t device,
                                        lpvs_problem **out);
int32_t lpvs_problem_create_lpv_f32(const float *y, const float *X, const float *V, int64_t N,
                                    const float *w, int64_t Nf, int64_t Nv, int32_t normalize,
                                    int32_t coulomb, int32_t device, lpvs_problem **out);
int32_t lpvs_problem_create_lpv_multi_f32(const float *Y, int64_t ns, const float *X, const float *V, int64_t N, const float *w,
                                          int64_t Nf, int64_t Nv, int32_t normalize, int32_t coulomb, int32_t device,
                                          lpvs_problem **out);
/* lpvs_windows_estimate_f64 for Float32 callers (float in / out, double arithmetic) */
int32_t lpvs_windows_estimate_f32(const float *Y, int64_t ns, const float *t, int64_t L, int64_t n, int64_t noverlap,
                                  const float *W, const float *freqs, int64_t Nf, int32_t estimator, double lam,
                                  int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol, int64_t iters,
                                  int32_t linear_sign, int64_t win_lo, int64_t win_hi, int32_t device, float *x_re, float *x_im,
                                  int64_t *iters_out);
/* lpvs_windows_estimate_multi_f64 / lpvs_windowcsd_f64 / lpvs_problem_create_lpv_rows_f64 / lpvs_problem_solve_ridge_f64 /
 * lpvs_admm_set_state_f64 for Float32 callers */
int32_t lpvs_windows_estimate_multi_f32(const float *Y, int64_t ns, const float *t, int64_t L, int64_t n, int64_t noverlap,
                                        const float *W, const float *freqs, int64_t Nf, int32_t estimator, double lam,
                                        int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol,
                                        int64_t iters, int32_t linear_sign, const int32_t *devices, int32_t ngpus, float *x_re,
                                        float *x_im, int64_t *iters_out);
int32_t lpvs_windowcsd_f32(const float *y, const float *u, const float *t, int64_t L, int64_t n, int64_t noverlap,
                           const float *W, const float *freqs, int64_t Nf, int32_t estimator, double lam, int32_t prox_kind,
                           double prox_param, int64_t group_len, double mu, double tol, int64_t iters, int32_t linear_sign,
                           int64_t win_lo, int64_t win_hi, int32_t device, float *Syu_re, float *Syu_im, float *Syy,
                           float *Suu, float *x_re, float *x_im, int64_t *iters_out);
int32_t lpvs_problem_create_lpv_rows_f32(const float *Y, int64_t ns, const float *X, const float *V, int64_t N_local,
                                         const float *w, int64_t Nf, int64_t Nv, int32_t normalize, int32_t coulomb,
                                         const double *ranges4, int32_t device, lpvs_problem **out);
int32_t lpvs_problem_solve_ridge_f32(lpvs_problem *h, double ridge, float *x_out);
int32_t lpvs_admm_set_state_f32(lpvs_problem *h, const float *x, const float *z, const float *u, int64_t iters_done);
int32_t lpvs_admm_init_f32(lpvs_problem *h, const float *x0, double mu, double tol,
                           int32_t linear_sign);
int32_t lpvs_admm_get_f32(lpvs_problem *h, float *x_out, float *z_out, float *u_out);
int32_t lpvs_problem_get_params_f32(lpvs_problem *h, int32_t which, float *re_out, float *im_out);
int32_t lpvs_ls_spectral_f32(const float *y, const float *t, int64_t N, const float *f, int64_t Nf,
                             double lam, int32_t device, float *re_out, float *im_out);

/* ---- a15 window bookkeeping (DSP.arraysplit as used by src/windows.jl:27-36) ---------- */
int32_t lpvs_window_count(int64_t L, int64_t n, int64_t noverlap, int64_t *count);
int32_t lpvs_window_offsets(int64_t L, int64_t n, int64_t noverlap, int64_t *offsets /* 0-based */,
                            int64_t capacity, int64_t *count);
/* merge (src/windows.jl:57-70): yf is count x n (window-major, row w = window w) -> ym[L] */
int32_t lpvs_merge_f64(const double *yf, int64_t count, int64_t n, int64_t noverlap, int64_t L,
                       double *ym);

/* ---- batched windows: ls_windowpsd(y,t,freqs; estimator = ls_sparse_spectral)  ----------------------
 * src/lsfft.jl:112-126 driving src/lasso.jl:105-126 for every window of src/windows.jl:27-36, all windows
 * [win_lo, win_hi) (0-based, of the k = (L-n) div (n-noverlap) + 1 windows) solved together on `device`:
 * one batch of regressor panels, Gram matrices, factorisations and ADMM iterations per launch instead of a
 * sequential loop.  Windows are independent, so ranks of a multi-GPU job take disjoint [win_lo, win_hi).
 *   W          n window weights (NULL = rect/ones); the estimator is always the weighted 4-argument method
 *   linear_sign LPVS_LINEAR_QUADRATIC_AS_WRITTEN reproduces Quadratic(Q, q=+A'Wy) of src/lasso.jl:119-121
 *   prox_kind  L1, L0, GROUP_L2 or BALL_L0 (README.md:79-83; one workgroup per window selects its r largest)
 *   x_re,x_im  (win_hi-win_lo) x Nf, window-major: fourier2complex(z) of each window
 *   S_out      Nf: sum over these windows, in window order, of |x|^2 (NOT yet divided by k^2); may be NULL
 *   iters_out  per-window iteration count (stops per window at ||x-z|| < tol); may be NULL */
int32_t lpvs_windowpsd_sparse_f64(const double *y, const double *t, int64_t L, int64_t n, int64_t noverlap,
                                  const double *W, const double *freqs, int64_t Nf, int32_t prox_kind,
                                  double prox_param, int64_t group_len, double mu, double tol, int64_t iters,
                                  int32_t linear_sign, int64_t win_lo, int64_t win_hi, int32_t device,
                                  double *x_re, double *x_im, double *S_out, int64_t *iters_out);

/* phase times of the calling thread's last batched-window call (HIP events on the library's stream), out[0..9]:
 * Gram + rhs ms, inverse ms, ADMM / dense-solve ms, windows, batch mat-vec microseconds per launch (only when the environment
 * has LPVS_WINDOW_MATVEC_TIMING: 200 extra launches after the last pass), windows of that pass, passes, Gram form (0 dense, 1 structured with direct
 * slot sums, 2 structured with the slot sums by non-uniform FFT), bytes of packed inverses one iteration's launch reads, 1 if the pass ran one launch per iteration, 2 if that launch reads 32 of the
 * fixed-point tiles' 36 bits (the stale nibble product, LPVS_STORAGE_MIXED32: the default) (the timed launches are then the stand-alone batch
 * mat-vec of the two-launch scheme: the same product without the update, all 36 bits);
 * out[10..11] (when n_out >= 12): after lpvs_windows_estimate_multi_*: ranks of the RCCL communicator that gathered the
 * coefficients (0 = no collective ran: one device, or shards sharing a device), devices driven */
int32_t lpvs_windowpsd_last_timing(double *out, int32_t n_out);

/* estimator of the batched-window engine */
#define LPVS_EST_SPARSE 1 /* ls_sparse_spectral(y,t,f,W): Quadratic(Q,q) + ADMM        src/lasso.jl:105-126 */
#define LPVS_EST_DENSE 2  /* ls_spectral(y,t,f,W): (A'WA + lam I) \ A'Wy               src/lsfft.jl:74-80  */
#define LPVS_EST_SPARSE_INIT 3 /* ls_sparse_spectral(y,t,f,W; init=true): as LPVS_EST_SPARSE, started from
                                  fourier_solve(A,y,zerofreq,lam) = (A'A + lam^2 I) \ A'y -- the UNWEIGHTED ridge solution, as written (src/lasso.jl:112) */

/* ---- the engine itself: ns signals sharing the sampling points t (Y is L x ns column-major) --------------------------
 * Every window's Gram A'WA and factorisation are formed ONCE and serve all ns right-hand sides A'W y_s -- the y and u of
 * ls_windowcsd / ls_cohere (src/lsfft.jl:150-151,184-185 call the estimator twice per window on the same t).
 *   estimator   LPVS_EST_SPARSE (prox_*, mu, tol, iters, linear_sign as in lpvs_windowpsd_sparse_f64; lam unused),
 *               LPVS_EST_SPARSE_INIT (the same with init = true: lam = the lambda of the starting ridge solve) or
 *               LPVS_EST_DENSE (lam = ridge; the ADMM arguments are ignored)
 *   x_re, x_im  ns x (win_hi - win_lo) x Nf, signal-major then window-major: fourier2complex of every solution
 *   iters_out   ns x (win_hi - win_lo) iteration counts (0 for the dense estimator); may be NULL.  HOST memory only
 *               (as every int64_t* output of this header: iteration counts are bookkeeping the host loop consumes) */
int32_t lpvs_windows_estimate_f64(const double *Y, int64_t ns, const double *t, int64_t L, int64_t n, int64_t noverlap,
                                  const double *W, const double *freqs, int64_t Nf, int32_t estimator, double lam,
                                  int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol, int64_t iters,
                                  int32_t linear_sign, int64_t win_lo, int64_t win_hi, int32_t device, double *x_re,
                                  double *x_im, int64_t *iters_out);

/* The same call returning the raw ADMM state of every problem instead of the packed coefficients: the (x, z) that ADMM returns
 * (src/lasso.jl:170) and the scaled dual variable u (:147,:155), each ns x (win_hi - win_lo) x Nreg, signal-major then window-major,
 * Nreg = 2 Nf (2 Nf - 1 with the zero frequency first) in the reference's ordering [re; im] (src/lasso.jl:93-97).  Sparse estimators
 * only.  x_out / z_out / u_out are HOST arrays; any of them (and iters_out) may be NULL.  What the parity tests hold the window
 * batches' iteration to the oracle with (x, z AND u at the bench's own iteration count); fourier2complex(z) is what
 * lpvs_windows_estimate_f64 returns for the same arguments. */
int32_t lpvs_windows_estimate_state_f64(const double *Y, int64_t ns, const double *t, int64_t L, int64_t n, int64_t noverlap,
                                        const double *W, const double *freqs, int64_t Nf, int32_t estimator, double lam,
                                        int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol, int64_t iters,
                                        int32_t linear_sign, int64_t win_lo, int64_t win_hi, int32_t device, double *x_out,
                                        double *z_out, double *u_out, int64_t *iters_out);

/* ---- the same engine driven over several devices by ONE host process (SURVEY.md section 8(e) "Process model") --------
 * The k windows are split into contiguous ranges over `ngpus` devices (devices[r], or 0..ngpus-1 when devices == NULL;
 * ngpus <= 0: every visible device); one host thread, stream and engine pass per device, no data-path collective; the
 * per-window coefficients are gathered with ONE RCCL all-gather over xGMI (librccl.so.1 is bound at run time, only when
 * ngpus > 1) and returned for ALL k windows: x_re / x_im are ns x k x Nf, iters_out ns x k.  The caller accumulates
 * |x|^2 (src/lsfft.jl:122) or xy conj(xu) (:152, :187-189) in window order.  Window shards reproduce the single-device
 * run bit for bit (fixed segment lengths, one admission decision for the structured Gram).  Arguments may be host or
 * device pointers; device arguments are staged through the host once. */
int32_t lpvs_windows_estimate_multi_f64(const double *Y, int64_t ns, const double *t, int64_t L, int64_t n, int64_t noverlap,
                                        const double *W, const double *freqs, int64_t Nf, int32_t estimator, double lam,
                                        int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol,
                                        int64_t iters, int32_t linear_sign, const int32_t *devices, int32_t ngpus, double *x_re,
                                        double *x_im, int64_t *iters_out);

/* ---- multichannel LPV batches over several devices by ONE host process (BASELINE.json config 5) ------
 * Y is N x ns (one column per channel sharing X, V, w): the channels are split into contiguous ranges over `ngpus` devices
 * (devices[r], or 0..ngpus-1 when NULL; ngpus <= 0: every visible device), one host thread per device builds its shard's Gram and
 * factorisation ONCE and advances the shard's channels together (lpvs_problem_create_lpv_multi_f64); every channel stops at its own
 * ||x-z||_2 < tol.  No data-path collective.  prox as lpvs_problem_set_prox (the reference's ls_sparse_spectral_lpv is
 * LPVS_PROX_GROUP_L2 with group_len = 2 Nv, src/lasso.jl:53-55; BASELINE's cfg5 asks LPVS_PROX_BALL_L0, an extension).
 * re_out / im_out: (Nf*Nv) x ns column-major HOST arrays, channel q in column q, parameter index f + (v-1) Nf (src/lasso.jl:67-68);
 * iters_out: ns iteration counts (HOST, may be NULL).  Inputs may be host or device pointers (staged through the host once). */
int32_t lpvs_lpv_batch_multi_f64(const double *Y, int64_t ns, const double *X, const double *V, int64_t N, const double *w, int64_t Nf,
                                 int64_t Nv, int32_t normalize, int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol,
                                 int64_t iters, const int32_t *devices, int32_t ngpus, double *re_out, double *im_out, int64_t *iters_out);

/* ---- independent LPV signals, several devices, several solves in flight per device (extension: BASELINE.json config 3 as a batch)
 * The loop  [ls_sparse_spectral_lpv(Y[:,q], X[:,q], V[:,q], w, Nv; ...) for q in 1:nsig]  (src/lasso.jl:27-70 per signal) inside the
 * library: every signal has its OWN X and V (N x nsig column-major, like Y), hence its own Gram, factorisation and ADMM run.
 * Contiguous signal ranges go to the devices (ngpus <= 0: every visible device; devices may be NULL); per device `in_flight` host
 * threads (1 .. 8) each solve one signal at a time on a handle and stream of their own -- the matrix-core-bound Gram and factorisation
 * of one solve run under the HBM-bound iterations of another (one MI355X at N = 2^20, n = 8192: 13.9 signals/s with in_flight = 1,
 * 16.4-16.8 with 2).  No collective.  Results do not depend on ngpus / in_flight.  re_out / im_out: (Nf*Nv) x nsig column-major HOST
 * arrays (signal q in column q, parameter index f + (v-1) Nf); iters_out: nsig iteration counts (HOST, may be NULL).
 * Y, X, V may be host or device pointers; a signal whose columns live on a device other than the one that solves it is copied there
 * (peer copy) by the constructor -- kernels never read another device's memory (this holds for every lpvs_problem_create_*). */
int32_t lpvs_lpv_signals_multi_f64(const double *Y, const double *X, const double *V, int64_t N, int64_t nsig, const double *w, int64_t Nf,
                                   int64_t Nv, int32_t normalize, int32_t prox_kind, double prox_param, int64_t group_len, double mu, double tol,
                                   int64_t iters, const int32_t *devices, int32_t ngpus, int32_t in_flight, double *re_out, double *im_out,
                                   int64_t *iters_out);

/* ---- ls_windowpsd_lpv                                                                    src/lsfft.jl:267-277
 * S[Nf] = sum over the windows of Windows3(Y, X, V, n, noverlap, rect), in window order, of abs2.(sum(reshape_params(x_i, Nf), dims=2))
 * with x_i = ls_spectral_lpv(y_i, x_i, v_i, w, Nv; lam, coulomb, normalize).x (:239-250: every window its own basis centres and Gram).
 * The windows' Grams are built `in_flight` (1 .. 8) at a time on streams of their own into ONE batch; their factorisations and
 * refined ridge solves then run for all windows at once (the batch machinery of the window engine).  n = length(Y) / nw as the caller
 * computes it (:269).  fva_out (HOST, k = window count entries, may be NULL): each window's fraction of variance explained
 * 1 - var(e)/var(y) (:255) -- the reference warns when it is below 0.9, the bindings do the same.  It is formed from the Gram
 * (x'Gx - 2x'b + y'y), i.e. from separately rounded sums: good to ~1e-8 of var(y), enough for the 0.9 threshold and no more; a constant
 * window (var(y) = 0) reports -Inf, so that it warns.  The windows are solved in chunks sized from the device's free memory; a window's
 * coefficients depend on the chunking to rounding only.
 * LPVS_ENUMERIC when a window's normal equations are singular to working precision (the reference's QR route is the wrapper's).
 * S_out: HOST array. */
int32_t lpvs_windowpsd_lpv_f64(const double *Y, const double *X, const double *V, int64_t N, const double *w, int64_t Nf, int64_t Nv,
                               int64_t n, int64_t noverlap, double lam, int32_t normalize, int32_t coulomb, int32_t device, int32_t in_flight,
                               double *S_out, double *fva_out);

/* ---- ls_windowcsd / ls_cohere on the engine                                              src/lsfft.jl:140-156, :176-193
 * Accumulators over the windows [win_lo, win_hi) in window order (NOT yet normalised: ls_windowcsd returns Syu / k,
 * ls_cohere |Syu|^2 / (Suu Syy)):  Syu += xy .* conj.(xu),  Syy += abs2.(xy),  Suu += abs2.(xu).  Any output may be NULL;
 * x_re / x_im (2 x nwin x Nf: xy of every window, then xu) and iters_out (2 x nwin) are optional. */
int32_t lpvs_windowcsd_f64(const double *y, const double *u, const double *t, int64_t L, int64_t n, int64_t noverlap,
                           const double *W, const double *freqs, int64_t Nf, int32_t estimator, double lam, int32_t prox_kind,
                           double prox_param, int64_t group_len, double mu, double tol, int64_t iters, int32_t linear_sign,
                           int64_t win_lo, int64_t win_hi, int32_t device, double *Syu_re, double *Syu_im, double *Syy,
                           double *Suu, double *x_re, double *x_im, int64_t *iters_out);

/* ---- storage of the inverse the ADMM mat-vec streams (after lpvs_admm_init) ------------------------------------------
 * *kind = 0 full symmetric doubles (n < 2048), 1 tile-packed lower triangle in doubles, 2 in floats (_f32 handles),
 * 3 in 6-byte elements (float head + 16-bit tail = 40 significant bits; LPVS_M_STORAGE=split, or a matrix of which fewer than
 * half of the tiles qualify for 4), 4 mixed: as 3, but tiles whose entries are all small against max|M| are 36-bit fixed point with a
 * per-row step (the default of _f64 handles -- with several right-hand sides the diagonal tiles always stay in the 6-byte format;
 * lpvs_admm_time_matvec reports the bytes a launch reads);
 * LPVS_M_STORAGE=f64 selects 1.  Bit 4 (+16) is set when, with the prox operator currently set, the ADMM iteration runs as ONE
 * launch (kind 4, one right-hand side, L1 / L0 / group prox whose groups divide 128: the tile partials are added into x with 64-bit
 * fixed-point atomics -- exact and order-independent -- and the next launch's tile workgroups apply prox and dual update in their
 * prologue); LPVS_ITERATION=two keeps the separate mat-vec and update launches.  Bit 5 (+32): the fixed-point tiles of kind 4 keep
 * 32 significant bits (4 B per element: handles whose x-update is corrected -- one right-hand side, n >= 2048 -- where the storage
 * error's systematic part leaves the iteration with the inverse's) */
int32_t lpvs_admm_matvec_kind(lpvs_problem *h, int32_t *kind);

/* ---- g1  autocov / autocor of a signal sampled at arbitrary times t                     src/autocov.jl
 * isequidistant (src/autocov.jl:112-121): t[1] - t[0] > 0 and abs(abs(t[i]-t[i-1]) - d) < 20d*eps() for every i, eps() of Float64.
 * N < 2 -> LPVS_EARGUMENT (the reference reads t[2]).  A device t is tested on its device, a host t on the host.
 *
 * lpvs_autofun: the nseg segments [seg_off[s], seg_off[s+1]) of t and y (seg_off: HOST, nseg+1 entries, seg_off[0] = 0, every segment
 * at least 2 samples) each take their own branch -- equidistant (src/autocov.jl:37-100: acf of the index lag j, lag sums accumulated
 * in double) or not (src/autocov.jl:125-175: y_i y_{i+j}, divided by var(y) for autocor, 1 where tau == 0) -- with the degenerate
 * rules (zeros / ones) of each.  Every pair (i, j >= 0, i+j < n) with NOT (tau > maxlag), tau = |t[i+j]-t[i]| in the eltype of t,
 * is returned, stably sorted by tau: the order of (tau, segment, enumeration index) that src/autocov.jl:1-12 produces (NaN maxlag
 * keeps every pair; NaN tau sorts last, as one canonical NaN).  normalize is used by the equidistant branch only.
 * Count protocol of lpvs_window_offsets: *count (HOST) is always set; tau_out = acf_out = NULL counts only; capacity < count ->
 * LPVS_EARGUMENT and nothing written.  Outputs (count elements each) may be host or device memory.  Output plus scratch that does not
 * fit in free device memory -> LPVS_ENOMEM (the pair count is in the message).  The _f32 twins take float t / y and return float tau /
 * acf (tau computed in float; lag sums and statistics in double). */
#define LPVS_ACF_COV 1
#define LPVS_ACF_COR 2
int32_t lpvs_isequidistant_f64(const double *t, int64_t N, int32_t *equidistant);
int32_t lpvs_isequidistant_f32(const float *t, int64_t N, int32_t *equidistant);
int32_t lpvs_autofun_f64(int32_t kind, const double *t, const double *y, const int64_t *seg_off, int64_t nseg, double maxlag,
                         int32_t normalize, int32_t device, double *tau_out, double *acf_out, int64_t capacity, int64_t *count);
int32_t lpvs_autofun_f32(int32_t kind, const float *t, const float *y, const int64_t *seg_off, int64_t nseg, double maxlag,
                         int32_t normalize, int32_t device, float *tau_out, float *acf_out, int64_t capacity, int64_t *count);
/* HIP-event phase times (ms) of the calling thread's last lpvs_autofun call, out[0..7]: statistics + row counts + scan (inputs
 * uploaded), lag sums + generation, sort, copy-out, total, pairs, sort passes, bytes per key */
int32_t lpvs_autofun_last_timing(double *out, int32_t n);

/* ---- g2  spectrogram / melspectrogram / mfcc                                       DSP.spectrogram, src/mel.jl
 * Host-only helpers, the reference's precision (Float32 unless Julia's promotion widens it):
 *   lpvs_nextfastfft: the smallest 2*3*5*7-smooth integer >= n (1 for n <= 1).
 *   lpvs_mel_filterbank (src/mel.jl:99-113): W, nmels x (nfft>>1)+1 floats, column-major.  wide bit0: fs was Float64 (the FFT grid is
 *     Float64), bit1 / bit2: fmin / fmax were Float64 (the mel grid is Float64); otherwise Int / Float32 arithmetic in Float32.
 *   lpvs_dct_matrix (src/mel.jl dct_matrix): D, nfilters x ninput floats, column-major, rows cos(i (1:2:2ninput) pi / 2ninput)
 *     sqrt(2/ninput), i = 1 .. nfilters (no DC row).
 * lpvs_stft: the frames of DSP.arraysplit (k = L >= n ? (L-n)/(n-noverlap) + 1 : 0; 0 <= noverlap < n else LPVS_EDOMAIN, nfft >= n),
 * windowed (window: n values or NULL), zero-padded to nfft, one-sided power with r = fs * sum(window.^2) (fs * n without a window):
 * row 0 |X_0|^2/r, rows 1 .. nfft/2-1 2|X_k|^2/r, the last row |X|^2/r for even nfft and 2|X|^2/r for odd.  Then by kind:
 *   LPVS_STFT_POWER  out = power, (nfft/2+1) x k;
 *   LPVS_STFT_MEL    out = W * power, nmels x k (W: nmels x (nfft/2+1), each band summed over its contiguous bins in ascending order;
 *                    a frame whose power holds a non-finite value is NaN in every band -- the reference's dense product);
 *   LPVS_STFT_MFCC   out = D * (W * power), each column divided by its 2-norm, nmfcc x k (no log; a zero column gives NaN).
 * All outputs column-major (rows x frames).  Count protocol of lpvs_window_offsets: *nframes (HOST) is always set, out = NULL counts
 * only, capacity < rows * k -> LPVS_EARGUMENT.  s, window, out may be host or device memory; W and D are host or device floats.
 * nfft: 7-smooth up to 8192 in LDS, 7-smooth above by a four-step FFT, any other by Bluestein; nfft (or its Bluestein length) beyond
 * 2^26 -> LPVS_EUNSUPPORTED.  Device arithmetic is double (the _f32 twins: float s / window / out); outputs plus the minimum scratch
 * that do not fit -> LPVS_ENOMEM.
 * lpvs_mel_project: out = W * power for a power matrix that already exists (nbins x frames, host or device), nmels x frames. */
#define LPVS_STFT_POWER 1
#define LPVS_STFT_MEL 2
#define LPVS_STFT_MFCC 3
int32_t lpvs_nextfastfft(int64_t n, int64_t *nfft);
int32_t lpvs_mel_filterbank(double fs, int64_t nfft, int64_t nmels, double fmin, double fmax, int32_t wide, float *W);
int32_t lpvs_dct_matrix(int64_t nfilters, int64_t ninput, float *D);
int32_t lpvs_stft_f64(int32_t kind, const double *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const double *window,
                      const float *W, int64_t nmels, const float *D, int64_t nmfcc, int32_t device, double *out, int64_t capacity,
                      int64_t *nframes);
int32_t lpvs_stft_f32(int32_t kind, const float *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const float *window,
                      const float *W, int64_t nmels, const float *D, int64_t nmfcc, int32_t device, float *out, int64_t capacity,
                      int64_t *nframes);
int32_t lpvs_mel_project_f64(const double *power, int64_t nbins, int64_t frames, const float *W, int64_t nmels, int32_t device, double *out);
int32_t lpvs_mel_project_f32(const float *power, int64_t nbins, int64_t frames, const float *W, int64_t nmels, int32_t device, float *out);
/* HIP-event times (ms) of the calling thread's last lpvs_stft call, out[0..8]: device work (Bluestein kernel, frame flags, FFTs,
 * epilogue), copy-out, total (setup + device work + copy-out), frames, path (1 LDS, 2 four-step, 3 Bluestein in LDS, 4 Bluestein
 * four-step), FFT length, frame pairs per workgroup (0 on the LDS fallback, which sends the power through global memory when the
 * epilogue's LDS regions do not fit next to one frame pair), output rows, setup (host tables, band ranges, uploads) */
int32_t lpvs_stft_last_timing(double *out, int32_t n);

/* ---- g2b  welch_pgram / periodogram and the heat-map quantile clamp          DSP.welch_pgram, DSP.periodogram, src/plotting.jl:38-47
 * lpvs_welch: the mean over the k frames of the one-sided power of lpvs_stft(LPVS_STFT_POWER, ...), S = (1/k) sum_f P_f: the same frames,
 * window, zero-padding, scale and doubling of the interior bins.  out: nfft/2+1 values, or nfft values when onesided == 0 (bins j and
 * nfft-j both hold the undoubled value; real input only).  L < n (no frame) -> LPVS_EDOMAIN; noverlap and nfft as lpvs_stft; *nframes
 * (HOST) is set to k.  No power matrix is written on the LDS paths: every workgroup adds the power columns of its frames in ascending
 * order into per-bin sums it keeps on the chip and writes one slab of partial sums; the slabs are added in a fixed pairwise tree (no
 * floating-point atomics: bitwise reproducible).  The longest chain of dependent additions behind one bin is out[9] of
 * lpvs_stft_last_timing (at most 1023 + ceil(log2 slabs)), the slabs out[10]; out[0..8] are set as by lpvs_stft.  s, window, out: host
 * or device memory.  A frame with a non-finite windowed sample makes every bin NaN; an all-zero frame adds exact zeros.
 * LPVS_STFT_WELCH names this epilogue inside the engine; lpvs_stft rejects it.
 * lpvs_compress: compress(x, q) of src/plotting.jl for the column-major sub-matrix x (rows x cols, leading dimension ld >= rows):
 * out = clamp(v, t0, t1) element by element with v = x (take_log == 0) or log(x) (logf for the _f32 twin), t0 / t1 the quantiles qlo /
 * qhi (swapped when qlo > qhi; outside [0, 1] -> LPVS_EARGUMENT) of all m = rows cols values v by Julia's default definition (type 7):
 * aleph = m p + (1 - p), j = clamp(trunc(aleph), 1, m-1), g = clamp(aleph - j, 0, 1), a = v_(j), b = v_(j+1) of the sorted values
 * (isless order: -0.0 < +0.0), a + g (b - a) if both are finite, else (1 - g) a + g b; m == 1 gives the element.  m == 0 or a NaN among
 * the values v (take_log: a NaN or a negative x) -> LPVS_EDOMAIN (Julia's quantile throws).  The order statistics come from an exact radix select on order-preserving
 * 64-bit keys (8-bit digits from the top, integer histograms), not from a sort.  _f32: the order statistics are the float values, the
 * interpolation runs in double, the output is float (a clamped element is the threshold rounded to float).  x and out (leading
 * dimension out_ld >= rows) may be host or device memory; thresholds (HOST, 2 doubles, may be NULL) receives t0, t1.
 * lpvs_compress_last_timing, out[0..4]: histogram passes, select ms, clamp ms, total ms, digits skipped (all surviving keys agreed). */
#define LPVS_STFT_WELCH 4
int32_t lpvs_welch_f64(const double *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const double *window, int32_t onesided,
                       int32_t device, double *out, int64_t *nframes);
int32_t lpvs_welch_f32(const float *s, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, double fs, const float *window, int32_t onesided,
                       int32_t device, float *out, int64_t *nframes);
int32_t lpvs_compress_f64(const double *x, int64_t rows, int64_t cols, int64_t ld, int32_t take_log, double qlo, double qhi, int32_t device,
                          double *out, int64_t out_ld, double *thresholds);
int32_t lpvs_compress_f32(const float *x, int64_t rows, int64_t cols, int64_t ld, int32_t take_log, double qlo, double qhi, int32_t device,
                          float *out, int64_t out_ld, double *thresholds);
int32_t lpvs_compress_last_timing(double *out, int32_t n);

/* ---- g3  ComplexNormal sampling and the Monte-Carlo bands of the SpectralExt recipe   src/utilities.jl:80-174, src/plotting.jl:54-97
 * Double precision only: the covariance of ls_spectral_lpv is always Float64, so these entry points have no _f32 twins.
 * All matrices column-major; V, R, Phi_g and the outputs may be host or device memory unless stated otherwise.
 *   lpvs_cholesky_upper_f64: U (n2 x n2, upper, strict lower triangle exactly zero) with U'U = V.  Only the upper triangle of V is
 *     read (Hermitian(...) is :U).  A pivot that is not positive -> LPVS_ENUMERIC with its 0-based index in lpvs_last_error (Julia's
 *     PosDefException); U_out is not written then.  Blocked, panels of 128, fixed summation order: bit-reproducible.
 *   lpvs_randn_f64: rows row0 .. row0+rows-1 and columns 0 .. cols-1 of the standard-normal matrix of `seed` (rows x cols).
 *     Element (i, j) depends on (seed, i, j) only: Philox4x32-10 with key (seed low word, seed high word) and counter (i low, i high,
 *     p low, p high), p = j / 2; from its words w0..w3: a = (w0 >> 5) 2^26 + (w1 >> 6), b = (w2 >> 5) 2^26 + (w3 >> 6),
 *     u1 = (a + 1) 2^-53 in (0, 1], r = sqrt(-2 log u1), t = b 2^-52 in [0, 2); column 2p is r cospi(t), column 2p+1 is r sinpi(t).
 *   lpvs_cov_f64: mean (cols) and corrected covariance (cols x cols, both triangles) of the columns of A (rows x cols, rows >= 2,
 *     cols <= 64), fixed-order reductions; mean_out and C_out are HOST arrays.
 *   lpvs_cn_create_f64: a handle (*cn, an id) of the distribution with mean m_re + i m_im (n each) and the real 2n x 2n covariance V
 *     in [re; im] order (the Sigma of ls_spectral_lpv); V is factored once and the factor stays on `device`.  lpvs_cn_destroy frees it
 *     (an unknown id is ignored).
 *   lpvs_cn_rand_f64: Z = m' .+ R U (src/utilities.jl:168-174), s draws: Z_re_out / Z_im_out are s x n (columns 1:n and n+1:2n).
 *     R (s x 2n) or NULL: the normals of lpvs_randn_f64(seed, 0, s, 2n), generated on the fly (seed is ignored when R is given).
 *   lpvs_cn_bands_f64: the draws of lpvs_cn_rand_f64(nMC), then for every frequency j < Nf and grid point i < G
 *     d = dot(z[j + v Nf], Phi_g[i, v]) over v < nb (Julia's dot: z conjugated; n = Nf nb, Phi_g is G x nb) for every draw,
 *     Fl / Fu = the 0-based order statistics nMC/10 - 1 and nMC - nMC/10 - 1 of |d|, Fm their mean (fixed-order sum); Pl / Pu / Pm the
 *     same of angle(d) when phase != 0 (else they may be NULL and are not written).  Outputs Nf x G.
 *     nMC < 10 -> LPVS_EARGUMENT (the reference indexes FB[:,:,0]); nMC > 16384 or nb > 1024 -> LPVS_EUNSUPPORTED (the draws of one
 *     cell are sorted in one workgroup's LDS).
 *   lpvs_cn_last_timing: HIP-event times (ms) of the calling thread's last calls, out[0..6]: factor (lpvs_cn_create_f64), sample,
 *     bands, sample + bands, 2n, draws, cells. */
int32_t lpvs_cholesky_upper_f64(const double *V, int64_t n2, int32_t device, double *U_out);
int32_t lpvs_randn_f64(int64_t seed, int64_t row0, int64_t rows, int64_t cols, int32_t device, double *R_out);
int32_t lpvs_cov_f64(const double *A, int64_t rows, int64_t cols, int32_t device, double *mean_out, double *C_out);
int32_t lpvs_cn_create_f64(const double *m_re, const double *m_im, const double *V, int64_t n, int32_t device, int64_t *cn);
int32_t lpvs_cn_destroy(int64_t cn);
int32_t lpvs_cn_rand_f64(int64_t cn, int64_t s, int64_t seed, const double *R, double *Z_re_out, double *Z_im_out);
int32_t lpvs_cn_bands_f64(int64_t cn, int64_t Nf, int64_t nb, const double *Phi_g, int64_t G, int64_t nMC, int64_t seed, const double *R,
                          int32_t phase, double *Fl, double *Fu, double *Fm, double *Pl, double *Pu, double *Pm);
int32_t lpvs_cn_last_timing(double *out, int32_t n);

/* ---- g4  generalised Lomb-Scargle periodogram of non-uniformly sampled signals (extension: the reference has none; the floating-mean
 * form of Zechmeister & Kuerster, A&A 496 (2009), without the time shift tau).
 * y: N x ns column-major (ns signals sharing the times t), W: N non-negative weights or NULL (ones), normalised to w = W / sum W;
 * f: Nf frequencies in cycles per unit of t.  The phase of (f_k, t_n) is phi = 2 pi (f_k t_n) with the EXACT product reduced to one
 * cycle before any trigonometry.  Per frequency  C = sum w cos, S = sum w sin, C2 = sum w cos 2phi, S2 = sum w sin 2phi;  per signal
 * Y = sum w y, YY = sum w y^2, YC = sum w y cos, YS = sum w y sin  (center_data: y is replaced by y - Y first; the weighted mean is
 * formed on the device in a fixed order).  CC = (1 + C2)/2, SS = (1 - C2)/2, CS = S2/2;  fit_mean: YY -= Y^2, YC -= Y C, YS -= Y S,
 * CC -= C^2, SS -= S^2, CS -= C S.  D = CC SS - CS^2,  p = (SS YC^2 + CC YS^2 - 2 CS YC YS) / D.
 *   power (Nf x ns column-major): LPVS_LOMB_STANDARD p / YY in [0, 1]; LPVS_LOMB_PSD p N / 2 (unit weights: the classical
 *     unnormalised periodogram).  A constant signal has standard power 0: with u = (N + 16) 2^-53 and R = sum w y^2 of the signal as
 *     given, p / YY is replaced by 0 when YY <= (center_data: u^2 R) + (fit_mean: 3 u YY before the fit_mean term) -- the rounding
 *     residue that centring and the subtraction of Y^2 leave of a constant signal.
 *   coef (3 x Nf x ns: planes a, b, c, each Nf x ns column-major; may be NULL): y ~ c + a cos phi + b sin phi,
 *     a = (SS YC - CS YS) / D, b = (CC YS - CS YC) / D, c = (the mean center_data removed) + (fit_mean: Y - a C - b S).
 *   sums (HOST, (4 + 2 ns) Nf + 3 ns doubles, may be NULL): the rows C, S, C2, S2, YC_0, YS_0, YC_1, ... of Nf values, then Y_c, YY_c
 *     per signal (of the centred signal, before the fit_mean terms), then the ns weighted means that center_data removed (as the
 *     device formed them; computed also when they are not removed).
 * Degenerate frequencies -- D <= 2^-40 (CC + SS)^2 with CC + SS taken before the fit_mean terms (f = 0, the Nyquist alias of a uniform
 * record) -- give power and coefficients 0 and are counted.  A non-finite t, y, W or f, a negative weight or sum W = 0 -> LPVS_EARGUMENT.
 * path: 0 auto, 1 direct sums (any grid), 2 non-uniform FFTs in blocks of modes (grids that are an arithmetic progression up to
 * rounding; LPVS_EARGUMENT otherwise).  Both paths add in a fixed order: two calls give the same bits, and a signal's column does not
 * depend on the other signals of the call.  t, y, W, power, coef: host or device memory; f, sums: host.
 * lpvs_lombscargle_last_timing (the calling thread's last call), out[0..11]: path taken, blocks of family 1 (C, S, YC, YS) and of
 * family 2 (C2, S2), fine grid (0: direct), degenerate frequencies, slabs of the direct sums, ms of the scan and the moments, the sums,
 * the epilogue, the copy-out, total, whether the first-order term of the frequency residuals ran. */
#define LPVS_LOMB_STANDARD 0
#define LPVS_LOMB_PSD 1
int32_t lpvs_lombscargle_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf,
                             int32_t fit_mean, int32_t center_data, int32_t normalization, int32_t path, int32_t device,
                             double *power, double *coef, double *sums);
int32_t lpvs_lombscargle_last_timing(double *out, int32_t n);

/* ---- g5  windowed Lomb-Scargle: the non-uniform twins of spectrogram and welch_pgram (extension).
 * y, t, W, f as in g4.  Window w < nwin is the contiguous index range [starts[w], starts[w] + counts[w]) of the record with the time
 * interval [lo[w], hi[w]] (starts, counts, lo, hi: HOST arrays).  Ranges may overlap, leave gaps, differ in length and come in any
 * order; counts[w] = 0 is allowed; a range outside [0, N], hi[w] < lo[w] or a non-finite lo / hi -> LPVS_EARGUMENT.
 * Window w is the g4 estimate of its own samples with the weights W_n g_w(t_n), the taper g_w evaluated from TIME, not from the index:
 *   LPVS_TAPER_RECT g = 1;  LPVS_TAPER_HANN g = sin^2(pi u), u = (t_n - lo_w) / (hi_w - lo_w), g = 0 for u outside [0, 1], g = 1 if
 *   hi_w == lo_w.  On a uniform record with lo = t[start], hi = t[start + count - 1] the Hann taper is DSP.hanning(count).
 * Everything else is g4 with N := counts[w]: the weights normalised by sum W g, the weighted mean formed on the device in a fixed order
 * and removed BEFORE the Fourier sums (center_data), the six sums per frequency and the moments per signal, the fit_mean terms, the
 * degenerate rule, the constant-signal rule with u = (counts[w] + 16) 2^-53, standard and psd (p counts[w] / 2) normalisation, phases
 * from the exact products f t.  An EMPTY window -- counts[w] = 0 or sum W g = 0, e.g. a Hann window whose only samples lie on its
 * edges -- is no error: its column of power and coefficients is 0, and it is counted and reported.
 *   power: average == 0: Nf x nwin x ns column-major (frequency fastest, then window, then signal); average == 1: Nf x ns, the mean of
 *     the window columns over the windows that are not empty, added in a fixed pairwise tree in the order of the list (0 if all are empty).
 *   coef (may be NULL; refused with average == 1): three planes a, b, c, each of the shape of the un-averaged power.
 *   empty_out (HOST, nwin int32, may be NULL): 1 for an empty window, else 0.
 * Errors as in g4: a non-finite t, y, W (anywhere in the record) or f, or a negative weight -> LPVS_EARGUMENT.  More than 2^24 windows,
 * Nf beyond 2^24, a window of more than 2^20 samples or a call whose work list exceeds a launch -> LPVS_EUNSUPPORTED.
 * Only direct sums: the transforms of g4 pay from 2^18 samples per transform on, and windows are far shorter.  A window's samples are
 * cut into slabs of a constant length, so every sum behind a window's column is added in an order that depends on that window alone:
 * two calls give the same bits, and a column does not depend on the other windows of the call, their order, or the other signals.
 * t, y, W, power, coef: host or device memory.
 * lpvs_lombscargle_windows_last_timing (the calling thread's last call), out[0..9]: windows, empty windows, work items (window slabs),
 * slab length, degenerate (window, frequency) pairs, ms of the scan and the moments, the sums, the epilogue (and the average), the
 * copy-out, total.
 * lpvs_time_windows_f64: the index ranges of the time intervals [lo[w], hi[w]] in a non-decreasing t (checked on the device;
 * LPVS_EARGUMENT otherwise, and for a non-finite t, lo or hi): starts_out[w] = #{t_n < lo_w}, counts_out[w] = #{t_n <= hi_w} - starts_out[w]
 * (0 when hi_w < lo_w), one device binary search per edge.  t: host or device memory; lo, hi, starts_out, counts_out: HOST. */
#define LPVS_TAPER_RECT 0
#define LPVS_TAPER_HANN 1
int32_t lpvs_lombscargle_windows_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf,
                                     const int64_t *starts, const int64_t *counts, const double *lo, const double *hi, int64_t nwin,
                                     int32_t taper, int32_t fit_mean, int32_t center_data, int32_t normalization, int32_t average,
                                     int32_t device, double *power, double *coef, int32_t *empty_out);
int32_t lpvs_lombscargle_windows_last_timing(double *out, int32_t n);
int32_t lpvs_time_windows_f64(const double *t, int64_t N, const double *lo, const double *hi, int64_t nwin, int32_t device,
                              int64_t *starts_out, int64_t *counts_out);

/* ---- g6  the bootstrap of the Lomb-Scargle periodogram: the maxima of the periodograms of B resamples of one record (extension; what
 * false-alarm probabilities and levels are read from without assuming Gaussian errors).
 * y: ONE signal of N samples; t, W, f and the flags as in g4.  Resample b >= 0 is y*_b[i] = y[pi_b(i)], t and W staying with the epochs
 * (under the null hypothesis the values are exchangeable and the weights belong to the times; astropy draws (y, dy) PAIRS instead, which
 * would make C, S, C2, S2 differ per resample: not done here).  The call computes the resamples row0 .. row0 + B - 1.
 * THE STREAM.  Philox4x32-10 keyed as lpvs_randn_f64 keys it: key = the 64-bit seed, counter = (b, pair p = i >> 1), words w0 .. w3;
 * sample 2p takes u = (w0 << 32) | w1, sample 2p + 1 takes u = (w2 << 32) | w3, and pi = (u N) >> 64, the high half of the 128-bit
 * product: pi < N always, the bias is below N 2^-64, and a resample depends on (seed, b) only.
 * Resample b's column of power IS the g4 estimate (same flags) of y[pi_b], t, W, f: the weights normalised by sum W, the weighted mean
 * formed on the device in a fixed order and removed before the Fourier sums, the fit_mean terms, the degenerate rule, the constant-signal
 * rule with N and the resample's own R and YY, phases from the exact products f t, both normalisations.
 *   max_out (B, host or device): the largest power of the resample's column.
 *   argmax_out (HOST, B int64, may be NULL): its frequency index; ties go to the lowest index.
 *   mean_out (HOST, B, may be NULL): the weighted mean of each resample as the device formed it (computed also when it is not removed).
 *   power_out (Nf x B column-major, host or device, may be NULL): the columns themselves, for small problems and tests; with NULL no
 *     B x Nf array exists anywhere, and no B x N array of resamples ever does.
 * FIXED ORDER.  Every sum is added in an order that depends on N and Nf only -- not on B, on row0, on how the call is cut into chunks, or
 * on whether power_out was asked for: two calls give the same bits, and resample b has the same bits alone (B = 1, row0 = b) and among
 * others.  Bit-equality with lpvs_lombscargle_f64 on the gathered signal is NOT promised (the additions come in another order).
 * Errors: a non-finite t, y, W or f, a negative weight, sum W = 0, B < 1, row0 < 0, N < 1, Nf < 1 -> LPVS_EARGUMENT; N >= 2^31,
 * Nf > 2^24, row0 + B > 2^40 or more resamples than one call takes (2^31 - 1) -> LPVS_EUNSUPPORTED.
 * lpvs_lombscargle_bootstrap_last_timing (the calling thread's last call), out[0..11]: resamples, chunks, resamples per thread (TS), slab
 * length, slabs, degenerate frequencies (counted once: they are those of the record), ms of the scan and the shared sums C, S, C2, S2,
 * of the resamples' moments, of the bootstrap sums, of the epilogue and the maxima, of the copy-out, total. */
int32_t lpvs_lombscargle_bootstrap_f64(const double *y, const double *t, int64_t N, const double *W, const double *f, int64_t Nf,
                                       int64_t B, int64_t seed, int64_t row0, int32_t fit_mean, int32_t center_data,
                                       int32_t normalization, int32_t device, double *max_out, int64_t *argmax_out, double *mean_out,
                                       double *power_out);
int32_t lpvs_lombscargle_bootstrap_last_timing(double *out, int32_t n);

/* ---- g7  Lomb-Scargle with several harmonics per frequency (extension; astropy's nterms, Palmer's fast chi^2): at every frequency
 *   y ~ c + sum_{h = 1 .. K} a_h cos(h phi) + b_h sin(h phi),  K = nterms in 1 .. 6,
 * in weighted least squares.  y, t, W, f, the phases phi = 2 pi (f t) of the exact products, center_data and the moments as in g4.
 * SUMS.  With w = W / sum W and y_c the (optionally centred) signal:
 *   C_m = sum w cos m phi, S_m = sum w sin m phi (m = 1 .. 2K; C_0 = 1, S_0 = 0);  YC_h = sum w y_c cos h phi, YS_h = sum w y_c sin h phi
 *   (h = 1 .. K);  Y = sum w y_c, YY = sum w y_c^2.  One sincospi per (sample, frequency); the harmonics follow by complex rotation.
 * NORMAL EQUATIONS.  Unknowns in the order (a_1, b_1, a_2, b_2, ...), n = 2K.  For the harmonics h and j:
 *   A[cos h, cos j] = (C_|h-j| + C_{h+j}) / 2,  A[sin h, sin j] = (C_|h-j| - C_{h+j}) / 2,  A[cos h, sin j] = (S_{h+j} + sgn(j - h) S_|j-h|) / 2,
 *   g = (C_1, S_1, C_2, S_2, ...),  b = (YC_1, YS_1, ...).  fit_mean eliminates the constant: A -= g g^T, b -= Y g, YY -= Y^2.
 *   For K = 1 these are g4's formulas.
 * FIT.  A = L D L^T in that order without pivoting (pivots d_j);  theta = A^-1 b,  p = b^T theta;
 *   power_out (Nf x ns column-major): LPVS_LOMB_STANDARD p / YY, and 0 under g4's constant-signal rule (the same threshold on YY);
 *     LPVS_LOMB_PSD p N / 2.
 *   coef_out (may be NULL): 2K + 1 planes of Nf x ns column-major: plane 2 (h - 1) = a_h, plane 2 (h - 1) + 1 = b_h, plane 2K = c,
 *     c = (the mean center_data removed) + (fit_mean: Y - g^T theta).
 *   sums_out (HOST, (4K + 2K ns) Nf + 3 ns doubles, may be NULL): rows of Nf values: row 2 (m - 1) = C_m, row 2 (m - 1) + 1 = S_m; for
 *     signal c and harmonic h rows 4K + 2K c + 2 (h - 1) + {0, 1} = YC_h, YS_h; then Y_c, YY_c per signal (of the centred signal, before
 *     the fit_mean term), then the ns weighted means as the device formed them.  With K = 1 both layouts are g4's.
 * DEGENERATE FREQUENCIES.  A frequency is degenerate when some pivot fails d_j > 2^-40 (the entries of A are on the scale of unit total
 * weight, as g4's rule assumes): power and all coefficients are 0 there, and it is counted once.  There is no separate rule for
 * N < 2K + 1: such a record is degenerate at every frequency through its pivots.  (For K = 1 the pivots are CC and D / CC where g4 tests
 * D against (CC + SS)^2: the same frequencies away from the threshold, not the same rule.)
 * Errors: nterms outside 1 .. 6 and every argument error of g4 -> LPVS_EARGUMENT; Nf beyond 2^24 or more rows of sums than one launch
 * takes -> LPVS_EUNSUPPORTED.
 * ONLY DIRECT SUMS.  Every harmonic m of a progression of frequencies is a progression itself and could take the non-uniform FFTs of
 * g4 -- 2K families of transforms instead of two; that is not built, and there is no path argument.  The windowed estimators (g5) and
 * the bootstrap (g6) stay single-term.
 * Every sum is added in a fixed order that depends on N and Nf alone: two calls give the same bits, and a signal's column does not
 * depend on the other signals of the call.  t, y, W, power_out, coef_out: host or device memory; f, sums_out: host.
 * lpvs_lombscargle_terms_last_timing (the calling thread's last call), out[0..9]: nterms, signals per thread of the sums kernel, slabs,
 * degenerate frequencies, ms of the scan and the moments, the sums, the epilogue, the copy-out, total, accumulators per thread. */
int32_t lpvs_lombscargle_terms_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf,
                                   int32_t nterms, int32_t fit_mean, int32_t center_data, int32_t normalization, int32_t device,
                                   double *power_out, double *coef_out, double *sums_out);
int32_t lpvs_lombscargle_terms_last_timing(double *out, int32_t n);

/* ---- g8  weighted wavelet Z-transform of non-uniformly sampled signals (extension; Foster, AJ 112, 1709, 1996): at every time tau_j and
 * frequency f_k the floating-mean sinusoid fit of g4 under Gaussian weights whose width is a fixed number of periods.
 * INPUTS.  y (N x ns column-major), t, W >= 0 (NULL: ones): as in g4; t must be non-decreasing (checked on the device, as
 *   lpvs_time_windows_f64 does).  f[Nf] (host): finite and > 0.  tau[Ntau] (host): finite, in any order, inside or outside the record.
 *   c > 0: the decay; Foster's 1 / (8 pi^2) makes the weight exp(-f^2 (t - tau)^2 / 2), one period per sigma.  radius[Nf] (host): each
 *   > 0 or +inf -- how far a cell reaches; the entry point takes radii and never a weight threshold (the binding's wwz_radius(f, c, wmin)
 *   = sqrt(log(1 / wmin) / c) / (2 pi f) is the usual choice, Foster's own program drops samples below wmin = 1e-9).
 * CELL (k, j).  Its samples are those with tau_j - radius_k <= t_n <= tau_j + radius_k, both edges formed in double exactly as written:
 *   start = #{t < lo}, count = #{t <= hi} - start by binary search on the device (the rule of lpvs_time_windows_f64).  The weight of
 *   sample n is g_n = exp(-a_k d_n^2), d_n = t_n - tau_j, with a_k formed once per frequency in double as  w = 6.283185307179586 * f_k,
 *   a_k = c * (w * w).  The cell IS the g4 estimate of its samples with the weights W_n g_n / sum W g, fit_mean always on (the constant
 *   is part of Foster's basis), the phases phi = 2 pi (f t) of the exact products, the degenerate rule and the constant-signal rule with
 *   N := count.  The sums are accumulated with the unnormalised W g and divided by sum W g at the end.
 *   center_data (default on) removes the RECORD's weighted mean (weights W) once, before anything else; it serves the numerics only: the
 *   floating mean makes every output but c invariant under it, and c has it added back.
 * OUTPUTS, Nf x Ntau x ns with the frequency fastest -- element (c Ntau + j) Nf + k -- unless said otherwise; host or device memory:
 *   power_out      p / YY (g4's standard normalisation), in [0, 1]
 *   amplitude_out  sqrt(a^2 + b^2): Foster's weighted wavelet amplitude (WWA)
 *   wwz_out        (Neff - 3) p / (2 (YY - p)): Foster's Z, an F-statistic of the fit
 *   neff_out       Nf x Ntau: Neff = (sum W g)^2 / sum (W g)^2, the effective number of samples
 *   coef_out       optional, three such planes a, b, c of  y ~ c + a cos 2 pi f t + b sin 2 pi f t  with the phase origin t = 0.  Foster's
 *                  basis {1, cos w (t - tau), sin w (t - tau)} spans the same space: power, amplitude, Z and c are the same, and his
 *                  coefficients are (a, b) rotated by the angle 2 pi f tau:  a' = a cos + b sin,  b' = b cos - a sin.
 *   count_out      optional, host int64, Nf x Ntau: the samples in reach
 *   empty_out      optional, host int32, Nf x Ntau: 1 for an empty cell
 * RULES.  Nothing returned is ever NaN.  An empty cell -- count = 0, or sum W g = 0 (or sum (W g)^2 = 0) by underflow -- gives exact zeros
 *   in every plane and is flagged; it is no error.  A degenerate cell (g4's rule) gives zeros and is counted.  Neff <= 3 gives wwz = 0:
 *   the F-statistic has no degrees of freedom left.  A standard power zeroed by the constant-signal rule gives wwz = 0.  YY - p not above
 *   that same threshold while YY is (a fit exact to rounding) gives wwz = +inf.
 * ERRORS.  LPVS_EARGUMENT: a non-finite t, y, W, f or tau; f <= 0; a negative weight; c <= 0 (or not finite); a radius that is NaN or
 *   <= 0; a decreasing t; N, Nf, Ntau < 1; ns outside 1 .. 65535.  LPVS_EUNSUPPORTED: more than 2^24 of Nf or Ntau; more cells or work
 *   items than one launch takes.
 * DETERMINISM, as everywhere in the family: two calls give the same bits, and the additions behind a cell happen in an order that depends
 *   on that cell's (start, count) and on N alone (sample lanes by the absolute index mod 4, stages of 256 and slabs at absolute
 *   multiples, the slab length a function of N; samples outside a cell are skipped, never added as zeros).  So a time has the same bits
 *   alone, among others and with the list permuted, and a signal has the same bits alone and among others.
 * lpvs_wwz_last_timing (the calling thread's last call), out[0..15]: Nf, Ntau, times and signals per thread of the sums kernel, work
 *   items, slab length, empty cells, degenerate cells, staged and useful (sample, frequency, time) triples, then milliseconds of the
 *   staging with the scan and the means, the ranges with the work list, the sums, the epilogue, the copy-out and the total. */
int32_t lpvs_wwz_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, const double *tau,
                     int64_t Ntau, double c, const double *radius, int32_t center_data, int32_t device, double *power_out, double *amplitude_out,
                     double *wwz_out, double *neff_out, double *coef_out, int64_t *count_out, int32_t *empty_out);
int32_t lpvs_wwz_last_timing(double *out, int32_t n);

/* ---- g9  box least squares periodogram of non-uniformly sampled signals (extension; Kovacs, Zucker & Mazeh, A&A 391, 369, 2002, in
 * its binned form): at every frequency the record is folded into nbins phase bins and every box of kmin .. kmax adjacent bins (wrapping)
 * is tried as a two-level model -- one level inside the box, one outside.  It finds transits, eclipses and periodic drop-outs, which no
 * number of harmonics of g7 describes.  No trigonometry: a histogram and a search.
 * INPUTS.  y (N x ns column-major), t, W >= 0 (NULL: ones): as in g4; t finite, in ANY order (nothing is sorted).  W has its
 *   inverse-variance meaning in depth_err_out.  f[Nf] (host): finite and > 0.  nbins in 8 .. 2048.  kmin[Nf], kmax[Nf] (host): the widths
 *   in bins per frequency, 1 <= kmin <= kmax <= nbins / 2.  min_count >= 1: the least number of samples inside AND outside a box.
 *   dips_only: keep only boxes whose level lies below the level outside.  center_data: remove the weighted mean first (0: ybar = 0).
 *   normalization: 0 standard, 1 chi2.
 * WEIGHTS AND CENTRING: g4's, by the same kernels: w = W / sum W, ybar_c = sum w y_c, wy = w (y - ybar_c).  YY_c = sum w (y - ybar_c)^2 has
 *   g4's terms wy_n (y_n - ybar_c), but they are added up as integers -- two 64-bit words per term, cut against the largest term
 *   (csrc/bls_plan.h) --, not in g4's tree: the sum of the rounded terms to two roundings, with the same bits in any order of the samples.
 * QUANTISATION.  qw_n = rint(w_n 2^60); per signal A_c = max_n |wy_n| and qy_n = rint(wy_n 2^shy_c), shy_c = 61 - ceil(log2 N) -
 *   (ilogb(A_c) + 1): no sum of any subset leaves 63 bits (the proof: csrc/bls_plan.h).  Everything up to the objective is then exact
 *   integer arithmetic.  With W == NULL the weight of a box is its integer count at the scale 1 / N and no weight is quantised.
 * FOLD.  Per (sample, frequency): p = f t, e = fma(f, t, -p), phi = (p - rint(p)) + e, plus 1 if negative -- the fractional part of the
 *   exact product --, bin = min(nbins - 1, (int)floor(phi nbins)).  Per frequency the histograms HW[b] = sum qw, HY_c[b] = sum qy_c and
 *   HC[b] = the count, by integer atomic adds: exact, whatever the order.
 * SEARCH.  Box (k, b), kmin <= k <= kmax, 0 <= b < nbins: the bins b .. b + k - 1, wrapping.  r, s, count: its integer sums; R, S: the
 *   integer totals of the histograms (not assumed to be 2^60 and 0).  A box is valid if count >= min_count and N - count >= min_count,
 *   r > 0 and R - r > 0 and, with dips_only, s / r < (S - s) / (R - r) -- decided exactly, as s (R - r) < (S - s) r in 128-bit integers.
 *   The objective, in double from the integers, each converted once, evaluated as written:
 *       dq = ((s * s) / r + (sc * sc) / rc) - (S * S) / R,     sc = S - s, rc = R - r in integers,
 *   and Delta = dq 2^(60 - 2 shy) (with W == NULL: (dq N) 2^(-2 shy)).  The best box has the largest dq; ties go to the smallest k, then
 *   to the smallest b.
 * OUTPUTS, Nf x ns column-major -- element c Nf + k:
 *   power_out       host or device: standard: min(1, Delta / YY), the share of the weighted variance the box explains (the twin of g4's
 *                   standard power); chi2: sum W Delta, the fall of chi^2 against the constant model (= snr^2 up to rounding)
 *   depth_out       host or device: (S - s) / (R - r) - s / r, positive for a dip
 *   depth_err_out   host or device: sqrt((1 / r + 1 / (R - r)) / sum W), r and R - r as shares of the total weight
 *   start_out, width_out   host int32: the best box's first bin and width in bins
 *   count_out       host int64: the samples inside it
 *   degenerate_out  optional, host int32: 1 where the rule below bit
 *   hist_out        optional, host int64, [Nf][1 + ns][nbins]: the raw integer histograms HW (with W == NULL: the counts), then HY_c
 *   hcount_out      optional, host int32, [Nf][nbins]: HC
 * RULES.  Nothing returned is ever NaN.  No valid box, a constant signal (A_c = 0), a YY within g4's constant-signal threshold
 *   (lomb_yy_noise) or a variance that overflows: zeros in every plane, flagged and counted as degenerate; it is no error.
 * WHAT THE RESULT MEANS.  Up to about a dozen double roundings the device returns the exact box least squares of the record whose w_n
 *   and w_n (y_n - ybar) are rounded to the quanta 2^-60 and 2^-shy <= A 2^-(60 - ceil(log2 N)): a sum of n terms is off by at most n / 2
 *   quanta.  For N = 2^20 the quantum of wy is at most A 2^-40 and a sum over the whole record is off by at most A 2^-21.
 * ERRORS.  LPVS_EARGUMENT: a non-finite t, y, W or f; f <= 0; a negative weight or weights that sum to 0; nbins outside 8 .. 2048;
 *   kmin < 1, kmin > kmax or kmax > nbins / 2; min_count < 1; a normalization other than 0 and 1; N, Nf < 1; ns outside 1 .. 65535.
 *   LPVS_EUNSUPPORTED: more than 2^30 samples or 2^24 frequencies.
 * DETERMINISM.  Two calls give the same bits.  A frequency is folded and searched from its own histograms alone: the same bits alone,
 *   among others and in a permuted list, however many frequencies share a workgroup.  A signal has the same bits alone and among
 *   others.  The sums -- histograms, and YY -- are integer sums: with W == NULL and center_data = 0 (nothing is summed in floating point
 *   before the quantisation) a permutation of the samples leaves every bit of every output as it was, under both normalisations.  With
 *   weights or centring, sum W and ybar are g4's tree sums in sample order: a permutation may move them, and the quantised record with
 *   them, by a rounding.
 * lpvs_bls_last_timing (the calling thread's last call), out[0..15]: frequencies per workgroup F, signals per pass TS, passes, LDS
 *   bytes of a workgroup, the shift of the weights (60; 0 with W == NULL), the smallest and the largest shy_c, degenerate (frequency,
 *   signal) pairs, boxes tried per signal, whether W was NULL, then milliseconds of the staging with the scan and the moments, the
 *   maxima and the quantisation, fold and search, the copy-out and the total, and Nf. */
int32_t lpvs_bls_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nbins,
                     const int32_t *kmin, const int32_t *kmax, int64_t min_count, int32_t dips_only, int32_t center_data, int32_t normalization,
                     int32_t device, double *power_out, double *depth_out, double *depth_err_out, int32_t *start_out, int32_t *width_out,
                     int64_t *count_out, int32_t *degenerate_out, int64_t *hist_out, int32_t *hcount_out);
int32_t lpvs_bls_last_timing(double *out, int32_t n);

/* ---- g10  fold statistics of non-uniformly sampled signals (extension): shape-agnostic period finders.  Phase dispersion minimisation
 * with covers (PDM; Stellingwerf, ApJ 224, 953, 1978), the analysis-of-variance periodogram (AOV; Schwarzenberg-Czerny, MNRAS 241, 153,
 * 1989: the same sums under another normalisation) and the conditional entropy (CE; Graham et al., MNRAS 434, 2629, 2013).  They find
 * signals that are periodic but neither sinusoidal (g4, g7) nor box-shaped (g9): sawtooth pulsators, eclipsing binaries with two unequal
 * minima, machinery with a repeating transient.  All are functions of g9's FOLD: p = f t, e = fma(f, t, -p), phi = (p - rint(p)) + e,
 * plus 1 if negative; the bin of n bins is min(n - 1, (int)floor(phi n)).
 * INPUTS of both.  y (N x ns column-major), t: as in g9 (finite, t in ANY order).  f[Nf] (host): finite and > 0.
 *
 * PDM / AOV (lpvs_pdm_f64).  W >= 0 (NULL: ones).  nbins = Nb >= 2, covers = Nc >= 1, nfine = Nb Nc in 2 .. 2048.
 * WEIGHTS, CENTRING, QUANTISATION: g9's, by the same kernels: w_n, wy_n = w_n (y_n - ybar_c), qw_n = rint(w_n 2^60), qy_n = rint(wy_n
 *   2^shy_c), and g9's order-free YY_c.  With W == NULL the weight of a bin is its integer count at the scale 1 / N.
 * BINS.  The record is folded into nfine fine bins (histograms HW, HY_c, HC by integer atomic adds).  Coarse bin m, m = 0 .. nfine - 1, is
 *   the Nc adjacent fine bins m .. m + Nc - 1, wrapping; cover m mod Nc is a partition of the period into Nb bins, and every cover is
 *   used.  r_m, s_m: the integer sums of coarse bin m (exact subset sums); R, S: the integer totals.
 * THE STATISTIC, in double from the integers, each converted once, evaluated as written:
 *       sb = (sum_{m : r_m > 0} (s_m * s_m) / r_m) / Nc - (S * S) / R,
 *   SB = sb 2^(60 - 2 shy) (with W == NULL: (sb N) 2^(-2 shy)), the between-bin sum of squares pooled over the covers, and
 *       explained = min(1, max(SB, 0) / YY),      nonempty = M = #{m : r_m > 0}   (a property of the fold: shared by the signals).
 *   THE ORDER OF THE SUM: thread tid of 256 adds the terms of its bins m = tid, tid + 256, ... ascending; the 64 values of a wave are added
 *   in a tree (lane l takes lane l + 32, then l + 16, 8, 4, 2, 1); the four wave sums as (W0 + W1) + (W2 + W3).
 * WHAT THE CALLER FORMS (the Python and Julia layers do): theta = (1 - explained) Nc (N - 1) / (Nc N - M), Stellingwerf's pooled s^2 /
 *   sigma^2 with the samples counted once per cover (small at a period); aov = explained / (1 - explained) (N - M) / (M - 1) for Nc = 1,
 *   the between / within F ratio (+inf where explained = 1).  Degenerate entries: theta = 1, aov = 0.
 * OUTPUTS.  explained_out: host or device, Nf x ns column-major (element c Nf + k); nonempty_out: host int32 [Nf]; degenerate_out: host
 *   int32, Nf x ns; hist_out: optional, host int64 [Nf][1 + ns][nfine], g9's layout over the fine bins; hcount_out: optional, host int32
 *   [Nf][nfine].
 * RULES.  Nothing returned is ever NaN.  A (frequency, signal) is degenerate -- explained = 0, flagged and counted, no error -- for a
 *   constant signal (g9's rule: A_c = 0, a YY within lomb_yy_noise, or a variance that overflows), when M <= Nc (every sample in one run
 *   of fine bins, N = 1 among them) and when Nc N <= M (no degree of freedom left within the bins).
 *
 * CONDITIONAL ENTROPY (lpvs_cent_f64).  Unweighted by definition: no W.  nbins in 2 .. 256 phase bins, mbins in 2 .. 64 value bins,
 *   nbins mbins <= 8192.
 * VALUE BINS.  Per signal ymin, ymax by integer atomic minima / maxima on an order-preserving key of the double (exact, order-free);
 *   den = ymax - ymin, u = (y - ymin) / den, j = min(mbins - 1, (int)floor(u mbins)), formed once per sample.  den = 0 (a constant signal)
 *   or not finite: every j = 0, H = 0, the signal is flagged degenerate.
 * THE STATISTIC.  n_ij: the samples in phase bin i and value bin j (32-bit integer counts), n_i = sum_j n_ij.  In double, each integer
 *   converted once:      H = (sum_{n_ij > 0} n_ij * log(n_i / n_ij)) / N        -- the Shannon entropy of the value bin given the phase
 *   bin, in nats; every term is >= 0; the period is at the MINIMUM of H.
 *   THE ORDER OF THE SUM: thread tid adds the terms of its cells q = i mbins + j = tid, tid + 256, ... ascending; then the same tree.
 *   The counts may be kept in 1, 2 or 4 private copies per (frequency, signal), merged by integer additions (the plan keeps one:
 *   csrc/fold_plan.h): the result does not depend on it.
 * OUTPUTS.  entropy_out: host or device, Nf x ns column-major; ylim_out: host, [ns][2] = ymin, ymax; degenerate_out: host int32 [ns];
 *   hist_out: optional, host int32 [Nf][ns][nbins][mbins].
 *
 * WHAT THE RESULTS MEAN.  pdm: up to a counted number of double roundings (csrc/fold_plan.h) the exact statistic of the record whose w_n
 *   and w_n (y_n - ybar) are rounded to g9's quanta.  conditional entropy: the counts are exact; H is within c 2^-53 (1 + H) of the
 *   entropy of the counts.
 * ERRORS.  LPVS_EARGUMENT: a non-finite t, y, W or f; f <= 0; a negative weight or weights that sum to 0; nbins, covers, mbins outside
 *   their ranges; N, Nf < 1; ns outside 1 .. 65535.  LPVS_EUNSUPPORTED: more than 2^30 samples or 2^24 frequencies.
 * DETERMINISM.  Two calls give the same bits; a frequency has the same bits alone, among others and in a permuted list; a signal has the
 *   same bits alone and among others.  A permutation of the samples changes no bit of ANY output of lpvs_cent_f64, and none of
 *   lpvs_pdm_f64's with W == NULL and center_data = 0 (with weights or centring sum W and ybar are g4's tree sums in sample order).
 * lpvs_pdm_last_timing / lpvs_cent_last_timing (the calling thread's last call), out[0..15]: frequencies per workgroup F, signals per pass
 *   TS, passes, LDS bytes of a workgroup, copies of the histogram (pdm: 1), the shift of the weights (60; 0 with W == NULL; cent: 0), the
 *   smallest and the largest shy_c (cent: 0, 0), degenerate (frequency, signal) pairs (cent: degenerate signals), whether the call was
 *   unweighted, then milliseconds of the staging with the scan (pdm: and the moments), the quantisation (cent: the extremes and the value
 *   bins), the fold with its epilogue, the copy-out and the total, and Nf. */
int32_t lpvs_pdm_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nbins,
                     int32_t covers, int32_t center_data, int32_t device, double *explained_out, int32_t *nonempty_out, int32_t *degenerate_out,
                     int64_t *hist_out, int32_t *hcount_out);
int32_t lpvs_pdm_last_timing(double *out, int32_t n);
int32_t lpvs_cent_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *f, int64_t Nf, int32_t nbins, int32_t mbins,
                      int32_t device, double *entropy_out, double *ylim_out, int32_t *degenerate_out, int32_t *hist_out);
int32_t lpvs_cent_last_timing(double *out, int32_t n);

/* ---- g11  CLEAN deconvolution of the spectrum of a non-uniformly sampled signal (extension; Roberts, Lehar & Dreher, AJ 93, 968, 1987).
 * Every estimator above treats a frequency on its own, and uneven sampling convolves every line with the spectral window: one sinusoid
 * shows as a forest of sidelobes and aliases.  CLEAN takes the dirty spectrum D and the window Wn and greedily subtracts the window's
 * response to the strongest line; what is left is a short list of complex components C and a residual R.  It is the greedy twin of g2's
 * sparse fit and needs no Gram and no factorisation.  Complex values are interleaved (re, im) doubles throughout.
 * GRID.  f_m = m df (the double product), m = 0 .. 2 K, K = Nf - 1.  D_k is used for k = 0 .. K, Wn_m for m = 0 .. 2 K, and
 *   Wn_{-m} = conj(Wn_m).  All index arithmetic is on m, never on rounded frequencies.
 * THE DIRTY STAGE (lpvs_dirty_spectrum_f64).  y (N x ns column-major), t, W >= 0 (NULL: ones), center_data, path: as in g4, through the
 *   same kernels: w = W / sum W, y_c = y - ybar (center_data) and
 *       Wn_m = sum_n w_n e^{-2 pi i f_m t_n} = (C_m, -S_m),     D_k = sum_n w_n y_c,n e^{-2 pi i f_k t_n} = (YC_k, -YS_k)
 *   are g4's sums C, S, YC, YS on the 2 Nf - 1 frequencies, with exact-product phases in g4's fixed order on the direct path and by its
 *   transforms on the NUFFT path (path 0 chooses as g4 does).  D_out: [ns][Nf] complex, Wn_out: [2 Nf - 1] complex; host or device.
 * ADMISSIBLE BINS.  den_p = 1 - (Re Wn_2p Re Wn_2p + Im Wn_2p Im Wn_2p); bin p is admissible iff den_p >= 2^-20.  This drops p = 0
 *   (Wn_0 = 1) and the Nyquist aliases of a uniform record; nothing else is special-cased.
 * THE LOOP (lpvs_clean_loop_f64), per signal, R = D and C = 0 to begin with; iteration i = 0 .. niter - 1:
 *   1. P_k = Re R_k Re R_k + Im R_k Im R_k.  p: the admissible bin of the largest P, the lowest index among equal ones (a NaN is never
 *      the largest).
 *   2. No admissible bin: stop, status 2 (empty).
 *   3. tol > 0 and P_p <= (tol tol) P0, P0 the P_p of iteration 0: stop, status 1 (tol).  tol = 0 never stops.
 *   4. With R_p = (r, q), Wn_2p = (u, v):   tr = r u + q v,  ti = r v - q u  (conj(R_p) Wn_2p),
 *      a = ((r - tr) / den_p, (q - ti) / den_p),   c = (gain Re a, gain Im a) = (cr, ci).
 *   5. C_p = C_p + c (componentwise).  (p, c) is entry i of the pick list.
 *   6. For every k = 0 .. K, with Wn_{k-p} = (a1, b1) (b1 negated where k < p) and Wn_{k+p} = (a2, b2):
 *          ur = (cr a1 - ci b1) + (cr a2 + ci b2),   ui = (cr b1 + ci a1) + (cr b2 - ci a2),   R_k = (Re R_k - ur, Im R_k - ui).
 *   7. The count runs out: status 0 (niter).
 *   Every product, sum and quotient is one rounded double operation, in the order written; nothing is fused.  The result therefore does
 *   not depend on how the arg-max is reduced, on the thread count or on where the residual lives.
 *   INPUTS: D [ns][Nf], Wn [2 Nf - 1] (one window for all signals), host or device; gain in (0, 2); 0 <= niter <= 2^24; tol in [0, 1).
 *   OUTPUTS: R_out, C_out: [ns][Nf] complex, host or device.  picks_out: host int32 [ns][niter], the bins in the order picked, -1 behind
 *   the last; pickval_out: [ns][niter] complex, host or device, the c of each pick, 0 behind the last; iters_out, status_out: host int32
 *   [ns], the picks made and why the loop ended.
 * RESTORATION (lpvs_clean_restore_f64).  B_m = exp(-(x x) / (2 (sigma sigma))), x = (double)m df: a real Gaussian beam, so phases refer
 *   to the epoch of t.   S_k = R_k + sum_p [C_p B_{k-p} + conj(C_p) B_{k+p}] over the p with C_p != 0 in increasing p, each term added as
 *   (Re C_p B_{|k-p|} + Re C_p B_{k+p}, Im C_p B_{|k-p|} - Im C_p B_{k+p}).  sigma > 0 is the caller's: the Python and Julia layers fit it
 *   to the window, sigma = h / sqrt(2 ln 2) with h the half-power half width of the main lobe -- the first m with |Wn_m|^2 < 1/2,
 *   interpolated linearly in |Wn|^2 (csrc/clean_plan.h: clean_sigma).  S_out: [ns][Nf] complex, host or device.
 * lpvs_clean_f64: the three stages in one call; D, Wn and R stay on the device between them.  sigma = 0 asks the library for the fit
 *   above; sigma_out (optional, host) receives the width used.  Every output has the bits the three separate calls give.
 * NOT COVERED: one signal is one workgroup (a lone signal uses one compute unit: the loop is bound by latency, and a barrier across
 *   workgroups would cost more than an iteration); beams other than the Gaussian; several harmonics per component (g7).
 * ERRORS.  LPVS_EARGUMENT: Nf < 2; niter < 0; gain outside (0, 2); tol outside [0, 1); df <= 0 or not finite; sigma <= 0 (restore) or < 0
 *   (clean) or not finite; N < 1; ns outside 1 .. 65535; a path other than 0, 1, 2; a non-finite t, y, W, D or Wn; a negative weight or
 *   weights that sum to 0.  LPVS_EUNSUPPORTED: Nf > 2^20; niter > 2^24; ns niter > 2^28.
 * DETERMINISM.  Two calls give the same bits; a signal has the same bits alone and among others.
 * lpvs_clean_last_timing (the calling thread's last call of any of the four; 0 where the call had no such stage), out[0..13]: the path
 *   of the sums (1 direct, 2 transforms), where the residual lived (1 LDS, 2 global memory), the threads of the loop's workgroup, its LDS
 *   bytes, the fewest and the most iterations of a signal, the admissible bins, then milliseconds of the staging with the scan and the
 *   moments, the sums, the loop, the restoration, the copy-out and the total, and sigma. */
int32_t lpvs_dirty_spectrum_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, double df, int64_t Nf, int32_t center_data,
                                int32_t path, int32_t device, double *D_out, double *Wn_out);
int32_t lpvs_clean_loop_f64(const double *D, int64_t ns, int64_t Nf, const double *Wn, double gain, int64_t niter, double tol, int32_t device,
                            double *R_out, double *C_out, int32_t *picks_out, double *pickval_out, int32_t *iters_out, int32_t *status_out);
int32_t lpvs_clean_restore_f64(const double *R, const double *C, int64_t ns, int64_t Nf, double df, double sigma, int32_t device, double *S_out);
int32_t lpvs_clean_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, double df, int64_t Nf, int32_t center_data,
                       int32_t path, double gain, int64_t niter, double tol, double sigma, int32_t device, double *D_out, double *Wn_out,
                       double *R_out, double *C_out, int32_t *picks_out, double *pickval_out, int32_t *iters_out, int32_t *status_out,
                       double *S_out, double *sigma_out);
int32_t lpvs_clean_last_timing(double *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* LPVSPECTRAL_H */
