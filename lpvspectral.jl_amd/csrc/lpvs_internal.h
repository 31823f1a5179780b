// lpvs_internal.h -- shared declarations of the gfx950 implementation behind include/lpvspectral.h
#pragma once
#include <hip/hip_runtime.h>
#include <exception>
#include <new>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/lpvspectral.h"
#include "windows_plan.h"
#include "admm_plan.h"
#include "gram_form_plan.h"
#include "eval_plan.h"
#include "lomb_plan.h"
#include "lomb_boot_plan.h"
#include "lomb_terms_plan.h"
#include "wwz_plan.h"
#include "bls_plan.h"
#include "fold_plan.h"
#include "clean_plan.h"
#include "pool_plan.h"

namespace lpvs {

// ---- environment knobs ------------------------------------------------------------------------------------------------------------
// Three kinds.  (1) Fallbacks of the OPTIONS of the interface (include/lpvspectral.h: LPVS_M_STORAGE, LPVS_ITERATION, LPVS_GRAM_FORM,
// LPVS_NT_LOADS, LPVS_NUDFT, LPVS_WINDOW_CHUNK_MB, LPVS_WINDOWS_IN_FLIGHT, LPVS_RESERVE_CUS, LPVS_XUPDATE_CORRECTION=0) and (2) operational
// ones that change no result (LPVS_POOL_GIB, LPVS_BATCH_PANEL_GIB, LPVS_TRACE, LPVS_NO_GRAPH, LPVS_WINDOW_MATVEC_TIMING, LPVS_MULTI_FORCE_RCCL,
// LPVS_MULTI_ALLOW_SHARED_DEVICE): plain getenv.  (3) EXPERIMENT knobs -- schedules and kernel variants kept for the A/B measurements the
// design documents quote, and the numerics studies (LPVS_FIX_BITS, LPVS_NIB_*, LPVS_TILE_ORDER, LPVS_NUFFT_SPREAD, LPVS_XB_REFINE, LPVS_XUPDATE_CORRECTION schedules, LPVS_PHASE,
// LPVS_FACTOR*, LPVS_PIVOT*, LPVS_KW, LPVS_LOOKAHEAD, LPVS_CHAIN, LPVS_BAND_TILE, LPVS_RU_STAGE, LPVS_MULTI_*, LPVS_POOL_FILL): read through experiment_env, which
// answers nullptr unless the process ALSO has LPVS_EXPERIMENTS=1 (the test-suite and tools/ set it; a production process that inherits a
// stray LPVS_FIX_BITS does not change its results), and is compiled out altogether with -DLPVS_NO_EXPERIMENTS.
inline const char *experiment_env(const char *name) {
#ifdef LPVS_NO_EXPERIMENTS
    (void)name;
    return nullptr;
#else
    const char *on = getenv("LPVS_EXPERIMENTS");
    return (on && on[0] == '1') ? getenv(name) : nullptr;
#endif
}

// ---- error plumbing ---------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define LPVS_HIP(call)                                                                       \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            lpvs::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                            __LINE__);                                                       \
            (void)hipGetLastError(); /* clear the sticky error state */                      \
            return e_ == hipErrorOutOfMemory ? LPVS_ENOMEM : LPVS_EDEVICE;                   \
        }                                                                                    \
    } while (0)
#define LPVS_TRY(call)                \
    do {                              \
        int32_t rc_ = (call);         \
        if (rc_ != LPVS_OK) return rc_; \
    } while (0)

// ---- options (include/lpvspectral.h LPVS_OPT_*; api.hip) ------------------------------------------------------------
// value in effect: the explicit value (a handle's, or a job's captured copy of its caller's defaults), else the calling thread's
// default, else what the environment variable of the same name says, else 0 (the library's own choice)
constexpr int kOptCount = 10;
int option_in_effect(int option, int explicit_value = 0);
void capture_default_options(int *opt /*[kOptCount]*/);
double infinity_cache_bytes();   // the device's last-level (Infinity) cache from the KFD topology, 256 MiB when it cannot be read   // the calling thread's defaults (for work handed to other threads)

// synchronises a stream when the scope is left: DevBufs declared BEFORE it return to the pool only after the stream is idle
struct DrainOnExit {
    hipStream_t s;
    explicit DrainOnExit(hipStream_t s_) : s(s_) {}
    ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};
// a call's own stream and its timing events, destroyed when the scope is left
struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};
template <int N> struct Events {
    hipEvent_t e[N] = {};
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// Body of a worker std::thread: an exception leaving it would end the process (std::terminate) -- it becomes a status instead.
template <class F, class OnFail>
static inline void run_guarded(F &&f, OnFail &&on_fail) {
    try { f(); }
    catch (const std::bad_alloc &) { set_error("out of host memory in a worker thread of the library"); on_fail(LPVS_ENOMEM); }
    catch (const std::exception &e) { set_error("worker thread of the library: %s", e.what()); on_fail(LPVS_EDEVICE); }
    catch (...) { set_error("worker thread of the library: unknown exception"); on_fail(LPVS_EDEVICE); }
}

// ---- device buffers ---------------------------------------------------------------------
// RAII device allocation; copy_in accepts a host or a device source pointer.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;   // true size of the block (>= the size asked for when it came from the cache)
    int dev = -1;
    int32_t alloc(size_t nbytes);
    void release();
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <class T> T *as() const { return static_cast<T *>(p); }
};
size_t pool_cached_bytes(int dev);   // bytes of freed blocks the caching allocator holds for a device (handed out again before hipMalloc is asked)
bool is_device_ptr(const void *p);
int device_of_ptr(const void *p);   // owning device, -1 for host memory
// dst device <- src (host or device); dst (host or device) <- src device
int32_t copy_to_device(void *dst_dev, const void *src, size_t bytes, hipStream_t s);
int32_t copy_from_device(void *dst, const void *src_dev, size_t bytes, hipStream_t s);
// a read-only argument made resident on device `dev` (aliased when it already is, or when there is nothing to stage)
template <class T> struct Staged {
    DevBuf own;
    const T *p = nullptr;
    int32_t set(const T *src, int64_t count, int dev, hipStream_t s) {
        if (!src || count == 0) { p = src; return LPVS_OK; }
        const int owner = device_of_ptr(src);
        if (owner == dev) { p = src; return LPVS_OK; }
        LPVS_TRY(own.alloc(sizeof(T) * (size_t)count));
        if (owner >= 0) {
            LPVS_HIP(hipMemcpyPeerAsync(own.p, dev, src, owner, sizeof(T) * (size_t)count, s));
            LPVS_HIP(hipStreamSynchronize(s));
        } else
            LPVS_TRY(copy_to_device(own.p, src, sizeof(T) * (size_t)count, s));
        p = own.as<T>();
        return LPVS_OK;
    }
};
// An output argument: device staging buffer when the caller's pointer is host memory.
struct DevOut {
    DevBuf own;
    double *p = nullptr;
    double *user = nullptr;
    size_t bytes = 0;
    int32_t set(double *dst, int64_t count) {
        user = dst; bytes = sizeof(double) * (size_t)count;
        if (is_device_ptr(dst)) { p = dst; return LPVS_OK; }
        LPVS_TRY(own.alloc(bytes));
        p = own.as<double>();
        return LPVS_OK;
    }
    int32_t finish(hipStream_t s) {
        if (p != user) return copy_from_device(user, p, bytes, s);
        LPVS_HIP(hipStreamSynchronize(s));
        return LPVS_OK;
    }
};
// body of every *_last_timing accessor: the first n of a thread's `count` timing slots
inline int32_t copy_timing(double *out, int32_t n, const double *slots, int32_t count) {
    if (!out || n < 0) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    for (int32_t k = 0; k < n && k < count; ++k) out[k] = slots[k];
    return LPVS_OK;
}

// ---- basis tables (basis.hip) -----------------------------------------------------------
// Fourier regressor, column-major N x Nreg (reference layout)          src/lsfft.jl:26-49
int32_t launch_fourier_regressor_colmajor(const double *t, int64_t N, const double *f, int64_t Nf,
                                          int zerofreq, double *A, hipStream_t s);
// Fourier regressor as a row-major panel P[n][ld] (k-major operand of the Gram kernel);
// columns >= Nreg up to ld are zero-filled.
int32_t launch_fourier_panel(const double *t, int64_t N, const double *f, int64_t Nf, int zerofreq,
                             double *P, int64_t ld, hipStream_t s);
// batch of window panels P[q][nrows][ld] (window q starts at sample toff[q], n samples, zero pad rows)
int32_t launch_window_panels(const double *t, const int64_t *toff_dev, int nbatch, int64_t n, int64_t nrows, const double *f,
                             int64_t Nf, int zerofreq, double *P, int64_t ld, hipStream_t s);
// trig table T[n][f] = (cos(w_f x_n), -sin(w_f x_n))                   src/lasso.jl:39
int32_t launch_trig_table(const double *X, int64_t N, const double *w, int64_t Nf, double2 *T,
                          hipStream_t s);
// activation table K[n][ldk] (row-major, nb valid entries per row)     src/lsfft.jl:195-207
int32_t launch_basis_table(const double *V, int64_t N, const double *vc, int64_t nb, double gamma,
                           int normalize, int coulomb, double *K, int64_t ldk, hipStream_t s);
// min / max / max|.| of V (device), results to host
int32_t device_minmax(const double *V, int64_t N, double *lo, double *hi, double *amax,
                      hipStream_t s);
// materialised LPV regressor, column-major N x 2*Nf*nb                 src/lasso.jl:35-50
int32_t launch_lpv_regressor_colmajor(const double2 *T, const double *K, int64_t ldk, int64_t N,
                                      int64_t Nf, int64_t nb, int permuted, double *Phi,
                                      hipStream_t s);
// column-major m x n -> k-major panel P[m][ld], pad columns zero-filled
int32_t launch_transpose_to_panel(const double *A, int64_t m, int64_t n, double *P, int64_t ld,
                                  hipStream_t s);

// ---- Gram (gram.hip) --------------------------------------------------------------------
// (GramPlan, make_gram_plan, make_gram_plan_pairs, gram_krs_fits, gram_stage_for: gram_form_plan.h)
// symmetric-pair form of the LPV Gram (see gram.hip): KK = pair products of the activation table
int32_t launch_pair_table(const double *K, int64_t ldk, int64_t nb, int64_t Npad, double *KK, hipStream_t s);
// (stage, where not NULL: the samples per stage of the gram_kernel instance that was launched)
int32_t launch_gram_krs(const GramPlan &pl, const double2 *T, int64_t Nf, const double *KK, int64_t nb,
                        double *slab, hipStream_t s, int *stage = nullptr);
int32_t launch_gram_reduce_krs(const GramPlan &pl, const double *slab, int64_t nb, double *G3, double *G,
                               int64_t ldg, hipStream_t s);
// Khatri-Rao form: Phi[k][f*2nb + c] = T[k][f][c>=nb] * K[k][c mod nb]
int32_t launch_gram_kr(const GramPlan &pl, const double2 *T, int64_t Nf, const double *K,
                       int64_t ldk, int64_t nb, double *slab, hipStream_t s, int *stage = nullptr);
// panel form: Phi[k][c] = P[k*ld + c], optional row weights W (applied once: G = P' diag(W) P)
int32_t launch_gram_panel(const GramPlan &pl, const double *P, int64_t ld, const double *W,
                          double *slab, hipStream_t s, int *stage = nullptr);
int32_t launch_gram_panel_batch(const GramPlan &pl, int nbatch, const double *P, int64_t batch_stride_P, int64_t ld,
                                const double *W, double *slab, hipStream_t s);
int32_t launch_gram_reduce_batch(const GramPlan &pl, int nbatch, const double *slab, double *G, int64_t ldg, hipStream_t s);
// G[a][b] (ldg x ldg, symmetric, full) = sum over chunks of the slabs
int32_t launch_gram_reduce(const GramPlan &pl, const double *slab, double *G, int64_t ldg,
                           hipStream_t s);
// b = Phi' (W .* y)
int32_t launch_rhs_kr(const double2 *T, int64_t Nf, const double *K, int64_t ldk, int64_t nb,
                      const double *y, int64_t N, double *b, double *scratch, size_t scratch_bytes,
                      hipStream_t s);
int32_t launch_rhs_panel(const double *P, int64_t ld, int64_t ncol, const double *W, const double *y,
                         int64_t N, double *b, double *scratch, size_t scratch_bytes, hipStream_t s);
size_t rhs_scratch_bytes(int64_t N, int64_t n);
int32_t launch_rhs_panel_batch(int nbatch, const double *P, int64_t strideP, int64_t ld, int64_t ncol, const double *W,
                               const double *y, const int64_t *yoff_dev, int64_t N, double *b, int64_t ldb, double *scratch,
                               size_t scratch_bytes, hipStream_t s);

// ---- structured Gram for arithmetic-progression frequency grids (nudft.hip) ----------------------------------
// (ApStep, ApSlots: gram_form_plan.h)
size_t nudft_partial_bytes(int64_t N, int64_t nslots, int64_t nq);
int64_t nudft_rows_per_chunk(int64_t N, int64_t nslots);
int32_t launch_nudft(const double *x, const double *y, int64_t N, const double *Wt, int64_t ldw, int nq, const double *om_hi,
                     const double *om_lo, int nslots, const ApStep &step, double *partial, double *tab, hipStream_t s);
// windows of one signal: seg_dev holds nwin*segs_per_window triples {first sample, end sample, first sample of the window}
int32_t launch_nudft_windows(const double *x, const double *y, const double *Wt, const double *om_hi, const double *om_lo, int nslots,
                             const ApStep &step, const int64_t *seg_dev, int nwin, int segs_per_window, double *partial, double *tab,
                             hipStream_t s);
// the same slot sums by a type-1 non-uniform FFT when the slot frequencies are j * D (nufft.hip); work: nufft_work_bytes
// (nufft_grid_size, nufft_applicable, nufft_windows_applicable: gram_form_plan.h)
size_t nufft_work_bytes(int64_t N, int64_t nslots, int64_t nq);
int32_t launch_nufft_tab(const double *x, const double *y, int64_t N, double xam, const double *Wt, int64_t ldw, int nq, double D_hi, double D_lo,
                         int mode0, int nslots, int nf, bool reuse_coords, void *work, double *tab, hipStream_t s);
constexpr int32_t kNufftNonFinite = -1000;       // launch_nufft_tab: a weight vector holds NaN / Inf -- take the direct sums (not an error)
std::vector<double> nufft_window_scale(int nf, int mode0, int nslots);
int32_t launch_nufft_window_spread(const double *x, const double *W, const double *yA, const double *yB, bool hasB, const int64_t *offs_dev, int nwin,
                                   int64_t n, double D_hi, double D_lo, int nf, double *gridA, double *gridB, int64_t grid_bstride, hipStream_t s);
int32_t launch_nufft_window_modes(const double *grids, int64_t grid_bstride, int nwin, int nf, int mode0, int nslots, const double *scale_dev, double *tab,
                                  int64_t tab_bstride, hipStream_t s);
// s0 = slot of the sum frequency 2a (sum of (f, f') = slot s0 + f + f'), delta = residual of 2a against that slot
int32_t launch_ap_assemble_fourier(const double *tab, const double *eps, int64_t Nf, int64_t s0, double delta, int zf, int64_t n, double *G,
                                   int64_t ldg, int nbatch, int64_t tab_stride, int64_t g_stride, hipStream_t s);
int32_t launch_ap_rhs_fourier(const double *tab, const double *eps, int64_t Nf, int zf, double *b, int nbatch, int64_t tab_stride,
                              int64_t b_stride, hipStream_t s);
int32_t launch_ap_assemble(const double *tab, const double *eps, int64_t Nf, int64_t s0, double delta, int64_t nb, int64_t n, double *G,
                           int64_t ldg, hipStream_t s);
int32_t launch_ap_rhs(const double *tab, const double *eps, int64_t Nf, int64_t nb, double *b, hipStream_t s);

// ---- model evaluation (eval.hip; the decisions: eval_plan.h) ---------------------------------------------------------------------------
// the basis of a call: vc = nb centres in device memory (nullptr: the Fourier family's single K = 1, nb = 1)
struct EvalBasis {
    const double *vc = nullptr;
    int nb = 1;
    double gamma = 0;
    int normalize = 0, coulomb = 0;
};
// out[c M + m] = s yhat_m[c] (y == nullptr) or y_m - s yhat_m[c]; part (or nullptr): 2 nc rows of eval_sum_slabs(M) partial sums.
// P_dev[(c nb + j) Nf + f] = (re, im) of p[f + j Nf, c]; w_dev: the angular frequencies whose ROUNDED products with x are the phases
int32_t launch_eval_direct(const double *x, const double *v, const double *y, int64_t M, const double *w_dev, int64_t Nf, const double *P_dev, int64_t nc,
                           const EvalBasis &B, double scale, double *out, double *part, hipStream_t s);
int32_t launch_eval_grids(const double *Q_dev, int64_t ngrids, int64_t Nf, int nf, double *tw_dev, double *grids_dev, hipStream_t s);
int32_t launch_eval_interp(const double *x, const double *v, const double *y, int64_t M, double a, double D_hi, double D_lo, int nf, const double *grids_dev,
                           bool twin, int64_t nc, const EvalBasis &B, double scale, double *out, double *part, hipStream_t s);
int32_t launch_eval_sums(const double *part, int64_t M, int64_t nc, double *sums_dev, hipStream_t s);

// ---- Lomb-Scargle periodogram (lomb.hip; the decisions: lomb_plan.h) ------------------------------------------------------------------------
// y, wy: [ns][N] (N x ns column-major); sums: [(4 + 2 ns)][Nf] rows C, S, C2, S2, YC_c, YS_c; power: Nf x ns column-major; coef: [3][ns][Nf]
int32_t launch_lomb_scan(const double *t, const double *y, const double *W, int64_t N, int64_t ns, int *flags_dev, double *part, double *sumW_dev, hipStream_t s);
int32_t launch_lomb_moments(const double *y, const double *W, int64_t N, int64_t ns, double sumW, bool center, double *w, double *wy, double *mean_dev,
                            double *mom_dev, double *part, hipStream_t s);
int32_t launch_lomb_direct(const double *t, const double *w, const double *wy, int64_t N, int64_t ns, const double *f_dev, int64_t Nf, const LombTiling &tl,
                           double *part, double *sums, hipStream_t s);
int32_t launch_lomb_slab_sum(const double *part, int64_t nslab, int64_t count, double *sums, hipStream_t s);
int32_t launch_lomb_prephase(const double *t, const double *w, const double *wy, int64_t N, int c0, int g, double base, bool prephase, double *Wt, hipStream_t s);
int32_t launch_lomb_combine(const double *tab, int nq, int nre, bool prephase, int count, int64_t k0, int64_t Nf, const double *eps_dev, double escale, int row0,
                            int c0, double *sums, hipStream_t s);
int32_t launch_lomb_epilogue(const double *sums, int64_t Nf, int64_t ns, const double *mom_dev, const double *mean_dev, bool fit_mean, bool center, bool psd,
                             int64_t N, double *power, double *coef, int *ndeg_dev, hipStream_t s);
// windows (lpvs_lombscargle_windows_f64; the work list: lomb_plan.h lomb_window_plan).  All pointers are device memory.
struct LombWindows {
    const double *t = nullptr, *y = nullptr, *W = nullptr;       // the record: t[N], y[ns][N], W[N] or nullptr
    int64_t N = 0, nwin = 0, nitems = 0;
    int ns = 0, taper = 0;
    const LombWindowItem *items = nullptr;                       // [nitems]
    const int64_t *starts = nullptr, *counts = nullptr, *offset = nullptr;   // [nwin]: first sample, samples, first item
    const int32_t *nslab = nullptr;                              // [nwin]
    const double *lo = nullptr, *hi = nullptr;                   // [nwin]: the time interval of the taper
};
// swg[nwin] = sum W g, mean[nwin][ns], mom[nwin][3 ns] = {Y_c, YY_c} per signal, then sum w y_c^2 of the signals as given; part: 3 ns nitems doubles
int32_t launch_lomb_windows_moments(const LombWindows &A, bool center, double *swg, double *mean, double *mom, double *part, hipStream_t s);
// sums[nwin][4 + 2 ns][Nf]; part: nitems (4 + 2 ns) Nf doubles
int32_t launch_lomb_windows_direct(const LombWindows &A, const double *f_dev, int64_t Nf, const LombTiling &tl, const double *swg, const double *mean_or_null,
                                   double *part, double *sums, hipStream_t s);
// power[ns][nwin][Nf], coef[3][ns][nwin][Nf] or nullptr, empty[nwin]; flags_dev |= 4: a window's weights do not sum to a finite value; ndeg_dev: zeroed here
int32_t launch_lomb_windows_epilogue(const LombWindows &A, const double *sums, int64_t Nf, const double *swg, const double *mom, const double *mean, bool fit_mean,
                                     bool center, bool psd, double *power, double *coef, int32_t *empty, int *flags_dev, unsigned long long *ndeg_dev, hipStream_t s);
// out[ns][Nf] = the mean of the columns cols[ns][nwin][Nf] of the windows that are not empty (0 if all are)
int32_t launch_lomb_windows_average(const double *cols, int64_t Nf, int64_t nwin, int64_t ns, const int32_t *empty, double *out, hipStream_t s);
// flags_dev (zeroed here) |= 1: a non-finite t, |= 8: t decreases somewhere; edges[2 w] = #{t < lo_w}, edges[2 w + 1] = #{t <= hi_w}
int32_t launch_lomb_time_windows(const double *t, int64_t N, const double *lo, const double *hi, int64_t nwin, int *flags_dev, int64_t *edges, hipStream_t s);

// bootstrap (lpvs_lombscargle_bootstrap_f64; lomb_boot.hip; the decisions: lomb_boot_plan.h).  All pointers are device memory; resamples are counted from row0.
// mean[B], mom[4 B] = {Y, YY of the resample less what centring removes, R = sum w y*^2, unused}; w: the normalised weights of the record
int32_t launch_lomb_boot_moments(const double *y, const double *w, int64_t N, int64_t seed, int64_t row0, int64_t B, bool center, double *mean, double *mom,
                                 hipStream_t s);
// sums[2 count][Nf] = YC, YS of the resamples r0 .. r0 + count - 1; part: plan.nslab * 2 count * Nf doubles
int32_t launch_lomb_boot_sums(const double *t, const double *w, const double *y, int64_t N, int64_t seed, int64_t row0, int64_t r0, int64_t count,
                              const double *mean_or_null, const double *f_dev, int64_t Nf, const LombBootPlan &plan, double *part, double *sums, hipStream_t s);
// shared[4][Nf] = C, S, C2, S2 of the record; power_or_null: Nf x B; maxv[B], maxi[B]; ndeg_dev += the degenerate frequencies when count_deg
int32_t launch_lomb_boot_epilogue(const double *shared, const double *sums, int64_t Nf, int64_t r0, int64_t count, const double *mean, const double *mom,
                                  bool fit_mean, bool center, bool psd, int64_t N, double *power_or_null, double *maxv, int64_t *maxi, bool count_deg, int *ndeg_dev,
                                  hipStream_t s);

// several harmonics per frequency (lpvs_lombscargle_terms_f64; lomb_terms.hip; the decisions: lomb_terms_plan.h).  All pointers are device memory.
// sums[(4K + 2K ns)][Nf]: rows C_m, S_m (m = 1 .. 2K), then YC_h, YS_h (h = 1 .. K) of every signal; part: pl.part_doubles doubles; w, wy: launch_lomb_moments'
int32_t launch_lomb_terms_sums(const double *t, const double *w, const double *wy, int64_t N, int64_t ns, const double *f_dev, int64_t Nf, const LombTermsPlan &pl,
                               double *part, double *sums, hipStream_t s);
// power[ns][Nf] (column-major Nf x ns), coef[2K + 1][ns][Nf] (a_h, b_h per harmonic, then c) or nullptr; ndeg_dev: one int, zeroed here
int32_t launch_lomb_terms_epilogue(int K, const double *sums, int64_t Nf, int64_t ns, const double *mom_dev, const double *mean_dev, bool fit_mean, bool center,
                                   bool psd, int64_t N, double *power, double *coef, int *ndeg_dev, hipStream_t s);

// weighted wavelet Z-transform (lpvs_wwz_f64; wwz.hip; the decisions: wwz_plan.h).  All pointers are device memory.
struct WwzArgs {
    const double *t = nullptr, *y = nullptr, *W = nullptr;       // the record: t[N], y[ns][N], W[N] or nullptr
    const double *mean = nullptr;                                // [ns]: the record's weighted means that are removed, or nullptr
    const double *f = nullptr, *decay = nullptr, *radius = nullptr;   // [Nf]
    const double *tau = nullptr;                                 // [ngroups TT]: the times in ascending order (WwzShape::tau_sorted)
    const int32_t *pos = nullptr;                                // [Ntau]: the place of the caller's time j in that order
    const WwzItem *items = nullptr;                              // [nitems]
    const int64_t *offset = nullptr, *first_slab = nullptr;      // [ngroups ftiles]: a pair's first item and the slab it covers
    int64_t N = 0, Nf = 0, Ntau = 0, nitems = 0, ftiles = 0, slab_samples = 0, rows = 0;
    int ns = 0, TT = 0;
};
int32_t launch_wwz_sorted(const double *t, int64_t N, int *flags_dev, hipStream_t s);
int32_t launch_wwz_ranges(const double *t, int64_t N, const double *a, const double *b, int64_t na, const double *r, int64_t nr, int64_t *edges, hipStream_t s);
// part: WwzWork::part_doubles doubles
int32_t launch_wwz_sums(const WwzArgs &A, int ts, double *part, hipStream_t s);
// power, amplitude, wwz[ns][Ntau][Nf], neff, count_out, empty_out[Ntau][Nf], coef[3][ns][Ntau][Nf] or nullptr; flags_dev |= 4: the weights of a cell do not sum
// to a finite value, |= 16: a cell outside its pair's items (never); counters[2] = {empty, degenerate cells}
int32_t launch_wwz_epilogue(const WwzArgs &A, const double *part, const int64_t *cell_edges, bool center, double *power, double *amplitude, double *wwz,
                            double *neff, double *coef, int64_t *count_out, int32_t *empty_out, int *flags_dev, unsigned long long *counters, hipStream_t s);

// box least squares periodogram (lpvs_bls_f64; bls.hip; the decisions: bls_plan.h).  All pointers are device memory.
struct BlsArgs {
    const double *t = nullptr;                                   // [N]
    const long long *qw = nullptr, *qy = nullptr;                // qw[N] (nullptr with unit weights), qy[ns][N]: the quantised record
    const double *f = nullptr;                                   // [Nf]
    const int32_t *kmin = nullptr, *kmax = nullptr;              // [Nf]: the widths in bins
    const int32_t *shy = nullptr;                                // [2 ns]: the shifts of the signals, then those of the terms of YY_c (or kBlsNoShift)
    const unsigned long long *amax = nullptr;                    // [2 ns]: the bit patterns of max |wy| (0: a constant signal), then of the largest term of YY_c
    const long long *yyacc = nullptr;                            // [2 ns]: the two integer words of YY_c (bls_plan.h: bls_yy)
    const double *mom = nullptr;                                 // launch_lomb_moments' mom_dev: sum w y_c^2 of the signal as given at 2 ns + c
    int64_t N = 0, Nf = 0, min_count = 1;
    int ns = 0, nbins = 0, dips_only = 1, chi2 = 0, center = 1, log2n = 0;
    double sumW = 1;
    double *power = nullptr, *depth = nullptr, *depth_err = nullptr;   // [ns][Nf]
    int32_t *start = nullptr, *width = nullptr, *degenerate = nullptr; // [ns][Nf]
    int64_t *count = nullptr;                                    // [ns][Nf]
    long long *hist = nullptr;                                   // [Nf][1 + ns][nbins] or nullptr
    int32_t *hcount = nullptr;                                   // [Nf][nbins] or nullptr
    unsigned long long *ndeg = nullptr;                          // the degenerate (frequency, signal) pairs
};
int32_t launch_bls_max(const double *y, const double *wy, const double *mean_dev, bool center, int64_t N, int64_t ns, unsigned long long *amax_dev, hipStream_t s);
int32_t launch_bls_quantise(const double *y, const double *w, const double *wy, const double *mean_dev, bool center, int64_t N, int64_t ns, int log2n,
                            const int32_t *shy_dev, const unsigned long long *amax_dev, long long *qw, long long *qy, long long *yyacc_dev, hipStream_t s);
int32_t launch_bls(const BlsArgs &A, const BlsPlan &plan, hipStream_t s);

// fold statistics (lpvs_pdm_f64, lpvs_cent_f64; fold.hip; the decisions: fold_plan.h).  All pointers are device memory.
struct PdmArgs {
    const double *t = nullptr;                                   // [N]
    const long long *qw = nullptr, *qy = nullptr;                // the quantised record, as BlsArgs has it
    const double *f = nullptr;                                   // [Nf]
    const int32_t *shy = nullptr;                                // [2 ns], as BlsArgs has them
    const unsigned long long *amax = nullptr;                    // [2 ns]
    const long long *yyacc = nullptr;                            // [2 ns]
    const double *mom = nullptr;                                 // launch_lomb_moments' mom_dev
    int64_t N = 0, Nf = 0;
    int ns = 0, nfine = 0, covers = 1, center = 1, log2n = 0;
    double *explained = nullptr;                                 // [ns][Nf]
    int32_t *nonempty = nullptr, *degenerate = nullptr;          // [Nf], [ns][Nf]
    long long *hist = nullptr;                                   // [Nf][1 + ns][nfine] or nullptr
    int32_t *hcount = nullptr;                                   // [Nf][nfine] or nullptr
    unsigned long long *ndeg = nullptr;                          // the degenerate (frequency, signal) pairs
};
int32_t launch_pdm(const PdmArgs &A, const PdmPlan &plan, hipStream_t s);
struct CentArgs {
    const double *t = nullptr, *f = nullptr;                     // [N], [Nf]
    const unsigned char *vbin = nullptr;                         // [ns][N]: the value bin of every sample
    const unsigned long long *lim = nullptr;                     // [2 ns]: the keys of ymin_c, then of ymax_c (fold_plan.h: fold_key)
    int64_t N = 0, Nf = 0;
    int ns = 0, nbins = 0, mbins = 0;
    double *entropy = nullptr;                                   // [ns][Nf]
    int32_t *hist = nullptr;                                     // [Nf][ns][nbins][mbins] or nullptr
};
// lim_dev[2 ns]: initialised here; then vbin[ns][N], ylim[ns][2] (doubles) and degenerate[ns]
int32_t launch_cent_prepare(const double *y, int64_t N, int64_t ns, int mbins, unsigned long long *lim_dev, unsigned char *vbin, double *ylim_dev,
                            int32_t *degenerate_dev, hipStream_t s);
int32_t launch_cent(const CentArgs &A, const CentPlan &plan, hipStream_t s);

// CLEAN (lpvs_dirty_spectrum_f64, lpvs_clean_loop_f64, lpvs_clean_restore_f64, lpvs_clean_f64; clean.hip; the decisions: clean_plan.h).
// All pointers are device memory; complex values are interleaved (re, im).
// sums: launch_lomb_direct's rows over the 2 Nf - 1 frequencies m df -> Wn[2 Nf - 1] = (C, -S), D[ns][Nf] = (YC_c, -YS_c)
int32_t launch_clean_repack(const double *sums, int64_t Nf, int64_t ns, double *Wn, double *D, hipStream_t s);
// flags_dev |= 1 where x[count] holds a value that is not finite
int32_t launch_clean_finite(const double *x, int64_t count, int *flags_dev, hipStream_t s);
// den[Nf], mask[Nf] (1: admissible), nadm_dev: zeroed here, then the count of the admissible bins
int32_t launch_clean_prologue(const double *Wn, int64_t Nf, double *den, unsigned char *mask, int *nadm_dev, hipStream_t s);
// R, C[ns][Nf] (C: zeroed by the caller), picks[ns][niter], pickval[ns][niter] (filled by the caller: only the picks made are written),
// iters, status[ns]; with the residual in global memory R is the working copy itself
int32_t launch_clean_loop(const double *D, const double *Wn, const double *den, const unsigned char *mask, int64_t ns, int64_t Nf, double gain, int64_t niter,
                          double tol, const CleanPlan &plan, double *R, double *C, int32_t *picks, double *pickval, int32_t *iters, int32_t *status, hipStream_t s);
// S[ns][Nf]; scratch: list[ns][Nf], count[ns], beam[2 Nf - 1]
int32_t launch_clean_restore(const double *R, const double *C, int64_t ns, int64_t Nf, double df, double sigma, int32_t *list, int32_t *count, double *beam,
                             double *S, hipStream_t s);

// ---- dense symmetric inverse (linalg.hip) ------------------------------------------------
// In-place inverse of the SPD matrix A (np x np, np % 64 == 0, full symmetric storage) by
// blocked symmetric sweeps; work holds 2 panels of np x 64 + one 64 x 64 block.
// Optional helper objects of the two-level sweep's look-ahead: the next pivot panel is prepared on a second
// (high-priority) stream while the bulk of the current trailing update runs on the caller's stream.
struct SweepAux {
    hipStream_t side = nullptr;
    hipStream_t bulk = nullptr;   // trailing updates of the pair schedule: a stream whose CU mask leaves a few CUs to the pivot chains (or nullptr)
    hipEvent_t panel = nullptr, rest = nullptr, band = nullptr, second = nullptr, bulkdone = nullptr;
    int32_t ensure();
    ~SweepAux();
};
size_t spd_inverse_work_bytes(int64_t np);
int32_t spd_inverse_inplace(double *A, int64_t np, double *work, int *status_dev, hipStream_t s, SweepAux *aux = nullptr);
int32_t launch_add_diag(double *M, int64_t np, int64_t n, double shift, hipStream_t s);
int32_t launch_add_diag_batch(double *M, int64_t np, int64_t n, double shift, int nbatch, hipStream_t s);
int32_t spd_inverse_inplace_batch(double *A, int64_t np, int nbatch, double *work, int *status_dev, hipStream_t s);
// C (m x m, ld) = A * B for symmetric np x np operands (test/diagnostic helper)
int32_t launch_symm_matmul(const double *A, const double *B, double *C, int64_t np, hipStream_t s);

// ---- ADMM (admm*.hip: the family map is at the head of admm.hip) --------------------------------------------------------------------
struct AdmmStatus {  // lives in device memory, copied back after each run
    long long iters;
    int converged;
    int pad;
    double nxz;
};
struct AdmmParams {
    const double *M;   // (G + I/mu)^-1, np x np
    int64_t np;        // padded size (multiple of 64)
    int64_t n;         // valid size
    const double *b;   // linear term (already signed)
    double *x, *z, *u, *rhs;
    double mu, tol;
    int prox_kind;
    double prox_param;
    int64_t group_len;
    AdmmStatus *status;
    double *scratch;   // >= 2*np doubles (top-r selection keys)
    double *part;      // symv_part_doubles(np) doubles of tile partials, or nullptr (full mat-vec)
    const double *Mp;  // tile-packed lower triangle of M (symv_packed_doubles(np)), or nullptr
    int ns;            // right-hand sides sharing M (signals of a shared-regressor batch); vectors are [ns][np]
    int mp_f32 = 0;    // Mp holds float (the _f32 entry points: M is streamed in single precision, arithmetic stays double)
    int mp_split = 0;  // Mp holds 6-byte elements (float head + 16-bit tail, 40 significant bits; see admm.hip)
    // 32-bit reads with a STALE NIBBLE PRODUCT (admm.hip, launch_nibble_refresh): the iteration streams the 32 leading bits of the fixed-point
    // tiles and the offset vector carries N rhs_g of the last refresh, xb = xb_corr + N rhs_g, re-formed after the launches g = 1 and g = 0 mod
    // nib_period.  nib_period = 0: off.  xb_corr: the offset vector without any nibble term; nib_rhs: np doubles of scratch.
    int nib_period = 0;
    int nib_ramp = 0;   // > 0: the first refreshes are denser -- the period is min(nib_period, max(1, 2^floor(log2 g) / nib_ramp)) (the right-hand side moves fastest in the first iterations)
    int mp_fix32 = 0;  // the fixed-point tiles keep 32 significant bits: their nibbles are zero and are not read (handles whose x-update is corrected: the storage error's systematic part leaves the iteration with the inverse's)
    const double *xb_corr = nullptr;
    double *nib_rhs = nullptr;
    long long *nib_acc = nullptr;   // np integers, zero between refreshes: the one-launch iteration's sums of the nibble planes' product (admm_iter_mixed_kernel<..., NIBR>)
    double *nib_part = nullptr;   // the nibble product's own per-tile partials (2 ntiles TS doubles: the two-launch iteration's are in flight in `part` when a refresh runs)
    // one prox parameter per signal slot (lpvs_problem_set_prox_per_signal): ns doubles in device memory, read through prox_param_of
    // (admm_device.h) by every update a handle with ns > 1 can reach; nullptr = prox_param for all (window batches and one-launch handles:
    // always).  It sits where mp_fix32 and its padding sat (mp_fix32 now fills the gap behind nib_ramp): the struct is a kernel argument,
    // and neither its size nor the offset of any other member has changed.
    const double *prox_params = nullptr;
    const unsigned char *mp_types = nullptr;   // mixed storage: per-tile format, 1 = 36-bit fixed point (admm.hip); several right-hand sides: diagonal tiles always 0
    // offset form of the x-update (single-problem tile-packed path): x = xb + M (z-u)/mu with xb = M b computed once from
    // the full-precision inverse; the per-iteration product then never multiplies the large constant vector b by the
    // reduced-precision copy of M (its rounding would otherwise be amplified by cond(G + I/mu)).  nullptr: x = M (b + (z-u)/mu).
    const double *xb = nullptr;
    // one-launch iteration (admm.hip): fixed-point accumulators, alternate u, per-parity block norms / maxima / quanta; nullptr = the
    // two-launch iteration.  fi_base = iterations committed before the chunk about to be launched.
    double *fi = nullptr;
    long long fi_base = 0;
    double fi_R = 0, fi_xbmax = 0;   // largest absolute row sum of M (x 1) and max|xb|: host copies of fi's constants (single problems)
    int fi_prefetch_all = 0;         // every tile is in the fixed format: diagonal tiles are requested up front too
    int tile_order = 0;              // 1: odd launches of a single problem walk the tiles below the diagonal in the mirrored order of tile_order.h (LPVS_TILE_ORDER)
    int opt_iteration = 0, opt_nt_loads = 0;   // LPVS_OPT_ITERATION / LPVS_OPT_NT_LOADS of the handle (0: thread default / environment)
    // one launch per iteration of the full-matrix path (np < kSymmetricMinNp; admm_small_iter_kernel): 4 ints per signal --
    // {converged before launch parity 0, parity 1, launch of the chunk that converged (-1: none), unused}; nullptr = two launches.
    // The alternate x / u buffers of that scheme are the two halves of `scratch`.
    int *sm_ctl = nullptr;
};
bool small_iter_applicable(const AdmmParams &p);
// xb (written) = xb_corr + N rhs, N = the nibble planes of the packed copy's fixed-point tiles; rhs = p.rhs (from_state = false) or (z - u_src) / mu
// (split: xb_corr (written) = xb - N rhs instead: after a correction re-formed xb for the right-hand side in memory)
int32_t launch_nibble_refresh(const AdmmParams &p, bool from_state, const double *u_src, hipStream_t s, bool split = false);
// (is it refreshed after launch g: nib_refresh_due of admm_plan.h)
// the one-launch iteration multiplies the nibble planes inside the launches after which a refresh is due (otherwise: launch_nibble_refresh's three kernels)
bool nib_fused_applies(const AdmmParams &p);
// one step of iterative refinement for the right-hand side the next x-update multiplies (p.rhs), its residual in twice-the-mantissa
// accumulation against H = G + shift I; xb_eff = xb0 + M~ (v - H M~ v).  t: 3 x [ns][np] scratch (admm.hip says why)
// b != NULL: for the whole right-hand side b + v, which also corrects an unrefined xb0 = M b
int32_t launch_xupdate_correction(const AdmmParams &p, const double *G, double shift, const double *b, const double *xb0, double *xb_eff, double *t, hipStream_t s);
size_t fi_doubles(int64_t np, int64_t nprob = 1);
bool fi_applicable(const AdmmParams &p);
int32_t launch_fi_setup(const AdmmParams &p, long long base, bool with_consts, hipStream_t s, double r_known = -1.0);   // r_known > 0: the largest absolute row sum is known (p.fi_R)
int32_t fi_read_consts(const AdmmParams &p, double out[2], hipStream_t s);
size_t symv_part_doubles(int64_t np, int64_t ns = 1);
size_t symv_packed_doubles(int64_t np);
int32_t launch_pack_tiles(const double *M, int64_t np, double *Mp, hipStream_t s);
int32_t launch_pack_tiles_f32(const double *M, int64_t np, float *Mp, hipStream_t s);
int32_t launch_pack_tiles_split(const double *M, int64_t np, unsigned char *Mp, hipStream_t s);   // 6 * symv_packed_doubles(np) bytes
int32_t launch_pack_tiles_mixed(const double *M, int64_t np, unsigned char *Mp, unsigned char *types, unsigned long long *absmax, hipStream_t s,
                                bool diag_float = false, double *abs_part = nullptr, int64_t n_valid = 0, double *rows_scratch = nullptr, int fix_bits = 36);   // diag_float: diagonal tiles always in the float-head format (multi-signal handles); abs_part: also the largest absolute row sum -> absmax[1]
bool multi_signal_fixed_tiles_ok(int64_t np);               // the multi-signal tile product in use reads fixed-point off-diagonal tiles
void release_panel_plans();                                 // admm_multi.hip: frees the cached device tables of the panel walk
int32_t launch_pack_tiles_mixed_batch(const double *M, int64_t np, int nbatch, unsigned char *Mp, unsigned char *types, unsigned long long *absmax,
                                      hipStream_t s, bool diag_float = false, double *abs_part = nullptr, int64_t n_valid = 0, double *rows_scratch = nullptr, int fix_bits = 36);
// (bytes read per tile of each format: kMixedFixedTileBytes, kMixedFixed32TileBytes, kMixedFloatTileBytes of windows_plan.h)
// element conversions for the _f32 entry points (device buffers)
int32_t launch_cvt_f32_f64(const float *src, double *dst, int64_t count, hipStream_t s);
int32_t launch_cvt_f64_f32(const double *src, float *dst, int64_t count, hipStream_t s);
// batch of nbatch independent problems of one shape: arrays are [nbatch][np]; matrices [nbatch / nrhs][np][np]
struct AdmmBatch {
    const double *M;
    int64_t np, n;
    int nbatch;
    const double *b;
    double *x, *z, *u, *rhs;
    double mu, tol;
    int prox_kind;
    double prox_param;
    int64_t group_len;
    AdmmStatus *status;   // [nbatch]
    double *part;         // symv_part_doubles(np, nbatch) doubles, zeroed before the first iteration (or nullptr)
    const double *Mp;     // [nbatch / nrhs] tile-packed lower triangles (or nullptr: plain mat-vec)
    int nrhs = 1;         // problems per matrix: problem q uses matrix q / nrhs (signals sharing a window's Gram)
    const double *xb = nullptr;   // offset form: x = xb + M~ (z-u)/mu, xb = M b per problem ([nbatch][np]); nullptr: classic
    const double *prox_params = nullptr;   // [nbatch] per-problem prox parameters (AdmmParams::prox_params; in mp_split's old place, as there); nullptr = prox_param for all
    const unsigned char *mp_types = nullptr;   // mixed storage: [matrix][tile] formats (1 = 36-bit fixed point), see admm.hip
    // one-launch iteration for the whole batch (admm.hip; nrhs == 1, mixed storage, offset form, fusable prox): fi_doubles(np, nbatch)
    // doubles of accumulators / records, iterations committed before the chunk about to be launched, "every tile is fixed point"
    double *fi = nullptr;
    long long fi_base = 0;
    int fi_prefetch_all = 0;
    int opt_iteration = 0, opt_nt_loads = 0;   // LPVS_OPT_ITERATION / LPVS_OPT_NT_LOADS of the call (0: thread default / environment)
    int mp_split = 0;                          // Mp holds 6-byte elements (float head + 16-bit tail)
    double *scratch = nullptr;                 // IndBallL0 with n > 8192: 2 * np doubles per problem (selection keys), else unused
    const double *x0 = nullptr;                // init = true: the starting point of every problem ([nbatch][np]); nullptr: zeros
    // 32-bit reads of the fixed-point tiles with the stale nibble product (AdmmParams: nib_period, nib_ramp, xb_corr, nib_acc), one-launch batches only:
    // xb is then written by the refreshes (xb = xb_corr + N rhs_g per problem), xb_corr keeps M b
    int nib_period = 0, nib_ramp = 0;
    const double *xb_corr = nullptr;           // [nbatch][np]
    long long *nib_acc = nullptr;              // [nbatch][np], zero between refreshes
};
bool fi_batch_applicable(const AdmmBatch &p);
// what the predicates of admm_plan.h read of a handle's / a batch's parameters (the iteration option is resolved per call: tests and
// tools switch it between handles); small_iter_applicable, fi_applicable, fi_batch_applicable and fused_ok are these plus the pure rule
inline IterFacts iter_facts(const AdmmParams &p) {
    IterFacts f;
    f.np = p.np; f.n = p.n; f.ns = p.ns; f.prox_kind = p.prox_kind; f.group_len = p.group_len;
    f.option_two = option_in_effect(LPVS_OPT_ITERATION, p.opt_iteration) == LPVS_ITERATION_TWO;
    f.packed = p.Mp != nullptr; f.partials = p.part != nullptr; f.offset = p.xb != nullptr; f.tile_formats = p.mp_types != nullptr;
    f.split_copy = p.mp_split != 0; f.f32_copy = p.mp_f32 != 0;
    f.fi = p.fi != nullptr; f.small_ctl = p.sm_ctl != nullptr; f.scratch = p.scratch != nullptr;
    return f;
}
inline IterFacts iter_facts(const AdmmBatch &p) {
    IterFacts f;
    f.np = p.np; f.n = p.n; f.ns = p.nbatch; f.prox_kind = p.prox_kind; f.group_len = p.group_len;
    f.option_two = option_in_effect(LPVS_OPT_ITERATION, p.opt_iteration) == LPVS_ITERATION_TWO;
    f.packed = p.Mp != nullptr; f.partials = p.part != nullptr; f.offset = p.xb != nullptr; f.tile_formats = p.mp_types != nullptr;
    f.split_copy = p.mp_split != 0; f.fi = p.fi != nullptr; f.scratch = p.scratch != nullptr;
    f.nrhs = p.nrhs; f.nbatch = p.nbatch;
    return f;
}
int32_t launch_fi_batch_setup(const AdmmBatch &p, hipStream_t s);   // constants and the records of iteration 0 (after launch_admm_batch_init)
bool admm_batch_uses_tiles(const AdmmBatch &p);   // will launch_admm_batch_iterations take the tile-packed path for this batch?
int32_t launch_batch_matvec(const double *A, int64_t np, int nprob, int nrhs, const double *v, double *out, hipStream_t s);   // out_q = A[q / nrhs] v_q
int32_t launch_pack_tiles_split_batch(const double *M, int64_t np, int nbatch, unsigned char *Mp, hipStream_t s);
int32_t launch_admm_batch_matvec_only(const AdmmBatch &p, int reps, hipStream_t s);
int32_t launch_batch_ridge_solve(const double *Q, const double *M, int64_t np, int64_t n, int nprob, int nrhs, const double *b, double ridge,
                                 int steps, double *x, double *t1, double *t2, hipStream_t s);
int32_t launch_pack_tiles_batch(const double *M, int64_t np, int nbatch, double *Mp, hipStream_t s);
int32_t launch_admm_batch_init(const AdmmBatch &p, hipStream_t s);
int32_t launch_admm_batch_iterations(const AdmmBatch &p, int64_t iters, hipStream_t s);
int32_t launch_admm_init(const AdmmParams &p, hipStream_t s);              // z=x, u=0, rhs, status=0
int32_t launch_admm_iterations(const AdmmParams &p, int64_t iters, hipStream_t s);
// resume: x, z, u hold saved iterates; recompute the next right-hand side, set the iteration count, clear the flags
int32_t launch_admm_restate(const AdmmParams &p, int64_t iters, hipStream_t s);
// the mat-vec kernel alone, `reps` times (x is recomputed from the current rhs; nothing else changes)
int32_t launch_admm_matvec_only(const AdmmParams &p, int reps, hipStream_t s);
int32_t launch_rect_matvec(const double *A, int64_t rows, int64_t cols, int64_t ld, const double *v, double *out, hipStream_t s);
int32_t launch_fourier_dual_panel(const double *t, int64_t N, const double *f, int64_t Nf, int zerofreq, double *D, int64_t ldn,
                                  int64_t nrows, hipStream_t s);
// x = M b refined against H = G + ridge I:  x += M (b - H x), `steps` times (t1, t2: np doubles of scratch)
int32_t launch_offset_vector_refined(const double *G, const double *M, int64_t np, int64_t n, int ns, const double *b, double shift, int steps,
                                     double *xb, double *t1, double *t2, hipStream_t s);
int32_t launch_ridge_solve_refined(const double *G, const double *M, int64_t np, int64_t n, const double *b, double ridge, int steps,
                                   double *x, double *t1, double *t2, hipStream_t s);
// x = Minv * rhs_in (one GEMV; ridge solves)
int32_t launch_symv(const double *M, int64_t np, const double *rhs, double *x, hipStream_t s, int ns = 1);   // x[q] = M rhs[q], q < ns

// ---- batched-window engine (api.hip) ------------------------------------------------------------------------------
struct WinJob {
    const double *const *ys; int64_t ns;          // ns signals sharing the sampling points t
    const double *t; int64_t L, n, noverlap;
    const double *W, *freqs; int64_t Nf;
    int estimator; double lam;                    // LPVS_EST_SPARSE / LPVS_EST_DENSE (ridge lam)
    int prox_kind; double prox_param; int64_t group_len; double mu, tol; int64_t iters; int linear_sign;
    int64_t win_lo, win_hi; int device;
    double t_absmax = -1.0;                       // max|t| over the WHOLE record when (t, L) is only a span of it (< 0: compute)
    bool f32_grid = false;                        // the frequency grid was widened from floats: snap it to the progression it was rounded from
    int opt[kOptCount] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // the caller's default options (captured on ITS thread: multi.hip runs the job on workers)
    bool opt_captured = false;
    // lpvs_windows_estimate_state_f64: the raw ADMM state (x, z, u of src/lasso.jl:146-155, reference ordering [re; im]) of every problem, written by the
    // pass that solved it into HOST arrays [ns][st_nwin][nreg] indexed by (window - st_base); any of the three may be null
    double *st_x = nullptr, *st_z = nullptr, *st_u = nullptr; int64_t st_base = 0, st_nwin = 0;
};
// sink(window index relative to win_lo, signal, re[Nf], im[Nf], iterations): window order, signals innermost
typedef std::function<void(int64_t, int64_t, const double *, const double *, int64_t)> WinSink;
int32_t windows_engine_run(const WinJob &job, const WinSink &sink, bool chunked = false);   // chunked: in cache-sized chunks, two parts of a chunk in flight (api.hip)
void windows_last_timing(double *out10);          // the calling thread's last engine call
void windows_set_timing(const double *in10);
void windows_set_multi_info(int rccl_ranks, int devices);   // out[10], out[11] of lpvs_windowpsd_last_timing

}  // namespace lpvs
