// uneven.hip -- the transforms of unevenly sampled records: lombscargle, its several-harmonic, windowed and bootstrap forms, wwz, bls and the
// fold statistics (pdm / aov, conditional_entropy).
// Host drivers and entry points; the kernels are in lomb.hip, lomb_terms.hip, lomb_boot.hip, wwz.hip, bls.hip and fold.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lpvs_internal.h"

using namespace lpvs;

namespace {

// ---- the front end of a call: what every transform of an uneven record does before its own kernels ----------------------------------------
// Timing events of a call on stream s: mark(i) records event i; finish() records the last one and synchronises, after which ms(i) is the
// time between the marks i and i + 1 and total() that between the first and the last.
template <int K> struct PhaseClock {
    Events<K> ev;
    hipStream_t s = nullptr;
    float gap[K - 1] = {}, all = 0;
    int32_t init(hipStream_t s_) {
        s = s_;
        for (auto &e : ev.e) LPVS_HIP(hipEventCreate(&e));
        return LPVS_OK;
    }
    int32_t mark(int i) { LPVS_HIP(hipEventRecord(ev.e[i], s)); return LPVS_OK; }
    int32_t finish() {
        LPVS_TRY(mark(K - 1));
        LPVS_HIP(hipStreamSynchronize(s));
        for (int i = 0; i + 1 < K; ++i) LPVS_HIP(hipEventElapsedTime(&gap[i], ev.e[i], ev.e[i + 1]));
        LPVS_HIP(hipEventElapsedTime(&all, ev.e[0], ev.e[K - 1]));
        return LPVS_OK;
    }
    double ms(int i) const { return gap[i]; }
    double total() const { return all; }
};

// what check() asks of the scan's sum of the weights
enum class WeightSum { positive, finite, unused };   // lombscargle, bls, pdm | wwz: a zero sum leaves every cell empty | windows: each window has its own

// The record (t[N], y[ns][N], W[N] or nullptr) of a call, resident on the device, and its small device record
//     [sum W | the weighted means: ns | launch_lomb_moments' moments: 3 ns | tail | flags word]
// (means and moments only when the call wants them).  The tail is the family's: as many 8-byte words as it asks for.  The flags word holds
// the int flags_dev and a spare int behind it (lombscargle's degenerate count).  Bits of the flags that check() answers for, whoever sets
// them: 1 a value that is not finite, 2 a negative weight (launch_lomb_scan), 8 t decreases (launch_wwz_sorted); 4 and 16 are the epilogues'
// and their drivers'.  A kernel of a new family that writes these flags keeps to that.
// A driver declares its Record with its other buffers, BEFORE its DrainOnExit, and calls the steps in this order; check() is a step of
// its own because wwz has its sortedness kernel write the flags first, and the windows read them only after their epilogue.
struct Record {
    int64_t N = 0, ns = 0;
    hipStream_t s = nullptr;
    Staged<double> t, y, W;
    DevBuf small, w, wy;                  // w, wy: the normalised weights and their products with the signals (moments())
    double *sumW_dev = nullptr, *mean_dev = nullptr, *mom_dev = nullptr;
    void *tail_ = nullptr;
    int *flags_dev = nullptr;
    double sumW = 0;                      // host copies, valid after check()
    int flags = 0;

    static int32_t admit(int device_) {
        if (lpvs_device_count() == 0) { set_error("no HIP device visible (the gfx950 path has no CPU fallback)"); return LPVS_EDEVICE; }
        LPVS_HIP(hipSetDevice(device_));
        return LPVS_OK;
    }
    int32_t stage(const double *t_, const double *y_, const double *W_, int64_t N_, int64_t ns_, int device, hipStream_t s_) {
        N = N_; ns = ns_; s = s_;
        LPVS_TRY(t.set(t_, N, device, s));
        LPVS_TRY(y.set(y_, N * ns, device, s));
        return W.set(W_, N, device, s);
    }
    int32_t alloc_small(size_t tail_words, bool moments = true) {
        const size_t shared = (size_t)(moments ? 1 + 4 * ns : 1);
        LPVS_TRY(small.alloc(sizeof(double) * (shared + tail_words + 1)));
        sumW_dev = small.as<double>();
        if (moments) { mean_dev = sumW_dev + 1; mom_dev = mean_dev + ns; }
        tail_ = sumW_dev + shared;
        flags_dev = reinterpret_cast<int *>(sumW_dev + shared + tail_words);
        return LPVS_OK;
    }
    template <class T> T *tail() const { return static_cast<T *>(tail_); }
    // part: lomb_sum_slabs(N) doubles of scratch; moments(), where it follows, wants 3 ns times as many of the same buffer
    int32_t scan(double *part) {
        return launch_lomb_scan(t.p, y.p, W.p, N, ns, flags_dev, part, sumW_dev, s);
    }
    int32_t check(const char *who, WeightSum rule) {
        if (rule != WeightSum::unused) LPVS_TRY(copy_from_device(&sumW, sumW_dev, sizeof(double), s));
        LPVS_TRY(copy_from_device(&flags, flags_dev, sizeof(int), s));
        if (flags & 1) { set_error("%s: t, y or W holds a value that is not finite", who); return LPVS_EARGUMENT; }
        if (flags & 2) { set_error("%s: a weight is negative", who); return LPVS_EARGUMENT; }
        if (flags & 8) { set_error("%s: t is not sorted (it decreases somewhere)", who); return LPVS_EARGUMENT; }   // (launch_wwz_sorted's)
        if (rule == WeightSum::unused) return LPVS_OK;
        if (!std::isfinite(sumW) || (rule == WeightSum::positive && !(sumW > 0.0))) { set_error("%s: the weights sum to %g", who, sumW); return LPVS_EARGUMENT; }
        return LPVS_OK;
    }
    int32_t moments(bool center, double *part) {
        LPVS_TRY(w.alloc(sizeof(double) * (size_t)N));
        LPVS_TRY(wy.alloc(sizeof(double) * (size_t)(N * ns)));
        return launch_lomb_moments(y.p, W.p, N, ns, sumW, center, w.as<double>(), wy.as<double>(), mean_dev, mom_dev, part, s);
    }
};

// ---- argument checks the entry points share ------------------------------------------------------------------------------------------------
int32_t host_frequencies(const double *f, int64_t Nf, std::vector<double> &hf) {
    hf.assign(f, f + Nf);
    for (double v : hf)
        if (!std::isfinite(v)) { set_error("lombscargle: a frequency is not finite"); return LPVS_EARGUMENT; }
    return LPVS_OK;
}
int32_t check_normalization(int32_t normalization) {
    if (normalization != LPVS_LOMB_STANDARD && normalization != LPVS_LOMB_PSD) { set_error("normalization must be 0 (standard) or 1 (psd), got %d", normalization); return LPVS_EARGUMENT; }
    return LPVS_OK;
}
// sums_out of lombscargle and its several-harmonic form: the nrow x Nf sums, then Y_c, YY_c per signal and the means of the record
int32_t copy_out_sums(double *sums_out, const DevBuf &dsums, int64_t nrow, int64_t Nf, const Record &rec) {
    if (!sums_out) return LPVS_OK;
    LPVS_TRY(copy_from_device(sums_out, dsums.p, sizeof(double) * (size_t)(nrow * Nf), rec.s));
    LPVS_TRY(copy_from_device(sums_out + nrow * Nf, rec.mom_dev, sizeof(double) * (size_t)(2 * rec.ns), rec.s));
    return copy_from_device(sums_out + nrow * Nf + 2 * rec.ns, rec.mean_dev, sizeof(double) * (size_t)rec.ns, rec.s);
}

// The sums of lombscargle over the frequencies hf -- rows C, S, C2, S2, YC_c, YS_c of `sums` -- of a record whose moments() have run, by
// the path lomb_choose_path takes: lombscargle's own, and the dirty stage of clean.  choose() admits the grid, decides and allocates the
// rows; run() launches.  Declared with the driver's other buffers, BEFORE its DrainOnExit.
struct LombSums {
    DevBuf sums, dfreq, dslab, dWt, dwork, dtab, deps;
    LombGrid lg;
    double tam = 0;
    int taken = 0, nf1 = 0;
    int64_t nblocks = 0, nslab = 0;
    bool twin = false;

    int32_t choose(const Record &rec, const std::vector<double> &hf, int32_t path) {
        const int64_t Nf = (int64_t)hf.size(), N = rec.N, nrow = 4 + 2 * rec.ns;
        if (lomb_needs_admission(path, N, Nf)) {         // not when the call goes direct whatever the grid is
            double tlo, thi;
            LPVS_TRY(device_minmax(rec.t.p, N, &tlo, &thi, &tam, rec.s));
            lg = lomb_admit(hf, tam);
        }
        taken = lomb_choose_path(path, lg.ok, N, Nf);
        if (taken == kLombPathRefused) {
            if (path != kLombPathNufft) set_error("path must be 0 (auto), 1 (direct) or 2 (NUFFT), got %d", path);
            else set_error("path = NUFFT but the frequency grid is not an arithmetic progression up to rounding (max|eps| = %.3g)", lg.emax);
            return LPVS_EARGUMENT;
        }
        return sums.alloc(sizeof(double) * (size_t)(nrow * Nf));
    }
    int32_t run(const Record &rec, const std::vector<double> &hf) {
        const int64_t Nf = (int64_t)hf.size(), N = rec.N, ns = rec.ns, nrow = 4 + 2 * ns;
        hipStream_t s = rec.s;
        if (taken == kLombPathDirect) {
            const LombTiling tl = lomb_tiling(N, Nf, ns);
            nslab = tl.nslab;
            LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
            LPVS_TRY(copy_to_device(dfreq.p, hf.data(), sizeof(double) * (size_t)Nf, s));
            LPVS_TRY(dslab.alloc(sizeof(double) * (size_t)(tl.nslab * nrow * Nf)));
            return launch_lomb_direct(rec.t.p, rec.w.as<double>(), rec.wy.as<double>(), N, ns, dfreq.as<double>(), Nf, tl, dslab.as<double>(), sums.as<double>(), s);
        }
        const char *knob = experiment_env("LPVS_LOMB_BLOCK");
        const int L = lomb_block_len(knob ? atoll(knob) : 0);
        const std::vector<LombBlock> blocks = lomb_blocks(hf, L);
        const std::vector<double> heps = lomb_block_residuals(hf, lg, L);
        for (double e : heps) twin = twin || e != 0.0;
        nblocks = (int64_t)blocks.size();
        const int nf = lomb_fine_grid(Nf, L), Lmax = (int)(Nf < L ? Nf : L);
        nf1 = nf;
        const int gmax = (int)(ns < kLombGroupSignals ? ns : kLombGroupSignals), nqmax = lomb_weight_vectors(1, gmax, true);
        LPVS_TRY(deps.alloc(sizeof(double) * (size_t)Nf));
        LPVS_TRY(copy_to_device(deps.p, heps.data(), sizeof(double) * (size_t)Nf, s));
        LPVS_TRY(dWt.alloc(sizeof(double) * (size_t)N * (size_t)nqmax));
        LPVS_TRY(dtab.alloc(sizeof(double) * 4 * (size_t)Lmax * (size_t)nqmax));
        LPVS_TRY(dwork.alloc(nufft_work_bytes(N, Lmax, nqmax)));           // (its fine grid is nf: that of the longest block)
        // family 1: step D, the weights w and w y_c of a group of signals; family 2: step 2D, w alone.  One set of sample coordinates per family.
        for (int family = 1; family <= 2; ++family) {
            const double w_hi = family == 1 ? lg.w1_hi : lg.w2_hi, w_lo = family == 1 ? lg.w1_lo : lg.w2_lo, fscale = family == 1 ? 1.0 : 2.0;
            bool have_coords = false;
            const int64_t ngroups = family == 1 ? lomb_signal_groups(ns) : 1;
            for (int64_t grp = 0; grp < ngroups; ++grp) {
                const int c0 = (int)(grp * kLombGroupSignals);
                const int g = family == 1 ? (int)(ns - c0 < kLombGroupSignals ? ns - c0 : kLombGroupSignals) : 0;
                for (const LombBlock &b : blocks) {
                    const int nq = lomb_weight_vectors(family, g, b.prephase), nre = 1 + g;
                    LPVS_TRY(launch_lomb_prephase(rec.t.p, rec.w.as<double>(), rec.wy.as<double>(), N, c0, g, fscale * b.base, b.prephase, dWt.as<double>(), s));
                    const int32_t rc = launch_nufft_tab(rec.t.p, nullptr, N, tam, dWt.as<double>(), nq, nq, w_hi, w_lo, 0, b.count, nf, have_coords, dwork.p,
                                                        dtab.as<double>(), s);
                    if (rc == kNufftNonFinite) { set_error("lombscargle: a weight vector of the transform is not finite"); return LPVS_ENUMERIC; }
                    LPVS_TRY(rc);
                    have_coords = true;
                    LPVS_TRY(launch_lomb_combine(dtab.as<double>(), nq, nre, b.prephase, b.count, b.k0, Nf, deps.as<double>(), fscale, family == 1 ? -1 : 2, c0,
                                                 sums.as<double>(), s));
                }
            }
        }
        return LPVS_OK;
    }
};

}  // namespace

// ---- Lomb-Scargle periodogram (lomb.hip; the decisions: lomb_plan.h) --------------------------------------------------------------------
// what lpvs_lombscargle_last_timing reports of the calling thread's last call: [0] path taken (1 direct, 2 transforms), [1], [2] blocks of
// family 1 / family 2 (0: direct), [3] fine grid (0: direct), [4] degenerate frequencies, [5] slabs of the direct sums (0: transforms),
// ms of [6] staging, the scan and the moments, [7] the sums, [8] the epilogue, [9] the copy-out, [10] total, [11] the first-order term ran
static thread_local double g_lomb_timing[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t lomb_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const std::vector<double> &hf, bool fit_mean, bool center,
                         bool psd, int32_t path, int32_t device, double *power, double *coef, double *sums_out) {
    const int64_t Nf = (int64_t)hf.size(), nrow = 4 + 2 * ns;
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dpower, dcoef;
    DevBuf dpart; LombSums ls;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    LPVS_TRY(dpower.set(power, Nf * ns));
    if (coef) LPVS_TRY(dcoef.set(coef, 3 * Nf * ns));
    // the small record has no tail; the degenerate count is the spare int of its flags word
    LPVS_TRY(rec.alloc_small(0));
    int *ndeg_dev = rec.flags_dev + 1;
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dpart.as<double>()));
    LPVS_TRY(rec.check("lombscargle", WeightSum::positive));
    LPVS_TRY(rec.moments(center, dpart.as<double>()));
    LPVS_TRY(ls.choose(rec, hf, path));
    LPVS_TRY(clock.mark(1));
    LPVS_TRY(ls.run(rec, hf));
    const DevBuf &dsums = ls.sums;
    const int taken = ls.taken, nf1 = ls.nf1;
    const int64_t nblocks = ls.nblocks, nslab = ls.nslab;
    const bool twin = ls.twin;
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_lomb_epilogue(dsums.as<double>(), Nf, ns, rec.mom_dev, rec.mean_dev, fit_mean, center, psd, N, dpower.p, coef ? dcoef.p : nullptr, ndeg_dev, s));
    LPVS_TRY(clock.mark(3));
    int ndeg = 0;
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(int), s));
    LPVS_TRY(copy_out_sums(sums_out, dsums, nrow, Nf, rec));
    LPVS_TRY(dpower.finish(s));
    if (coef) LPVS_TRY(dcoef.finish(s));
    LPVS_TRY(clock.finish());
    const bool nu = taken == kLombPathNufft;
    g_lomb_timing[0] = taken; g_lomb_timing[1] = (double)nblocks; g_lomb_timing[2] = (double)nblocks; g_lomb_timing[3] = nu ? nf1 : 0;
    g_lomb_timing[4] = ndeg; g_lomb_timing[5] = (double)nslab;
    for (int i = 0; i < 4; ++i) g_lomb_timing[6 + i] = clock.ms(i);
    g_lomb_timing[10] = clock.total();
    g_lomb_timing[11] = nu && twin ? 1 : 0;
    return LPVS_OK;
}

int32_t lpvs_lombscargle_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t fit_mean,
                             int32_t center_data, int32_t normalization, int32_t path, int32_t device, double *power, double *coef, double *sums) {
    try {
        if (!y || !t || !f || !power) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (N <= 0 || Nf <= 0 || ns <= 0 || ns > 65535) { set_error("need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = %lld, Nf = %lld, ns = %lld)", (long long)N, (long long)Nf, (long long)ns); return LPVS_EARGUMENT; }
        if (Nf > ((int64_t)1 << 24)) { set_error("%lld frequencies are too many", (long long)Nf); return LPVS_EUNSUPPORTED; }
        if (path < kLombPathAuto || path > kLombPathNufft) { set_error("path must be 0 (auto), 1 (direct) or 2 (NUFFT), got %d", path); return LPVS_EARGUMENT; }
        LPVS_TRY(check_normalization(normalization));
        if (is_device_ptr(f) || (sums && is_device_ptr(sums))) { set_error("lombscargle: f and sums are host memory"); return LPVS_EARGUMENT; }
        std::vector<double> hf;
        LPVS_TRY(host_frequencies(f, Nf, hf));
        return lomb_impl(y, ns, t, N, W, hf, fit_mean != 0, center_data != 0, normalization == LPVS_LOMB_PSD, path, device, power, coef, sums);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_lombscargle_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_lomb_timing, 12);
}

// ---- Lomb-Scargle with several harmonics per frequency (lomb_terms.hip; the decisions: lomb_terms_plan.h) ----------------------------------
// what lpvs_lombscargle_terms_last_timing reports of the calling thread's last call: [0] nterms, [1] signals per thread, [2] slabs,
// [3] degenerate frequencies, ms of [4] staging, the scan and the moments, [5] the sums, [6] the epilogue, [7] the copy-out, [8] total,
// [9] accumulators per thread
static thread_local double g_lomb_terms_timing[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t lomb_terms_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const std::vector<double> &hf, const LombTermsPlan &plan,
                               bool fit_mean, bool center, bool psd, int32_t device, double *power, double *coef, double *sums_out) {
    const int64_t Nf = (int64_t)hf.size(), nrow = plan.rows;
    const int K = plan.K;
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dpower, dcoef;
    DevBuf dpart, dsums, dfreq, dslab;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    LPVS_TRY(dpower.set(power, Nf * ns));
    if (coef) LPVS_TRY(dcoef.set(coef, (2 * K + 1) * Nf * ns));
    // the small record has no tail; the degenerate count is the spare int of its flags word
    LPVS_TRY(rec.alloc_small(0));
    int *ndeg_dev = rec.flags_dev + 1;
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dpart.as<double>()));
    LPVS_TRY(rec.check("lombscargle", WeightSum::positive));
    LPVS_TRY(rec.moments(center, dpart.as<double>()));
    LPVS_TRY(dsums.alloc(sizeof(double) * (size_t)(nrow * Nf)));
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, hf.data(), sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(dslab.alloc(sizeof(double) * (size_t)plan.part_doubles));
    LPVS_TRY(clock.mark(1));
    LPVS_TRY(launch_lomb_terms_sums(rec.t.p, rec.w.as<double>(), rec.wy.as<double>(), N, ns, dfreq.as<double>(), Nf, plan, dslab.as<double>(), dsums.as<double>(), s));
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_lomb_terms_epilogue(K, dsums.as<double>(), Nf, ns, rec.mom_dev, rec.mean_dev, fit_mean, center, psd, N, dpower.p, coef ? dcoef.p : nullptr, ndeg_dev, s));
    LPVS_TRY(clock.mark(3));
    int ndeg = 0;
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(int), s));
    LPVS_TRY(copy_out_sums(sums_out, dsums, nrow, Nf, rec));
    LPVS_TRY(dpower.finish(s));
    if (coef) LPVS_TRY(dcoef.finish(s));
    LPVS_TRY(clock.finish());
    double *g = g_lomb_terms_timing;
    g[0] = K; g[1] = plan.ts; g[2] = (double)plan.nslab; g[3] = ndeg; g[9] = plan.acc;
    for (int i = 0; i < 4; ++i) g[4 + i] = clock.ms(i);
    g[8] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_lombscargle_terms_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nterms,
                                   int32_t fit_mean, int32_t center_data, int32_t normalization, int32_t device, double *power_out, double *coef_out,
                                   double *sums_out) {
    try {
        if (!y || !t || !f || !power_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        const LombTermsPlan plan = lomb_terms_plan(N, Nf, ns, nterms);
        if (plan.status != kLombTermsOk) { set_error("%s", plan.why.c_str()); return plan.status == kLombTermsArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        LPVS_TRY(check_normalization(normalization));
        if (is_device_ptr(f) || (sums_out && is_device_ptr(sums_out))) { set_error("lombscargle: f and sums are host memory"); return LPVS_EARGUMENT; }
        std::vector<double> hf;
        LPVS_TRY(host_frequencies(f, Nf, hf));
        return lomb_terms_impl(y, ns, t, N, W, hf, plan, fit_mean != 0, center_data != 0, normalization == LPVS_LOMB_PSD, device, power_out, coef_out, sums_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_lombscargle_terms_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_lomb_terms_timing, 10);
}

// ---- windowed Lomb-Scargle (lomb.hip; the work list: lomb_plan.h lomb_window_plan) ----------------------------------------------------------
// what lpvs_lombscargle_windows_last_timing reports: [0] windows, [1] empty windows, [2] work items, [3] slab length, [4] degenerate
// (window, frequency) pairs, ms of [5] staging, the scan and the moments, [6] the sums, [7] the epilogue and the average, [8] the copy-out, [9] total
static thread_local double g_lomb_windows_timing[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t lomb_windows_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const std::vector<double> &hf,
                                 const std::vector<int64_t> &starts, const std::vector<int64_t> &counts, const double *lo, const double *hi, int taper,
                                 bool fit_mean, bool center, bool psd, bool average, int32_t device, double *power, double *coef, int32_t *empty_out) {
    const int64_t Nf = (int64_t)hf.size(), nrow = 4 + 2 * ns, nwin = (int64_t)counts.size();
    const LombWindowPlan plan = lomb_window_plan(counts);
    if (!plan.ok) { set_error("%s", plan.why.c_str()); return LPVS_EUNSUPPORTED; }
    const int64_t nitems = (int64_t)plan.items.size();
    if (!lomb_windows_fit(nitems, nwin, Nf, ns)) {
        set_error("lombscargle: %lld window slabs, %lld frequencies and %lld signals are more than one call takes", (long long)nitems, (long long)Nf, (long long)ns);
        return LPVS_EUNSUPPORTED;
    }
    const LombTiling tl = lomb_windows_tiling(Nf, ns);
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dpower, dcoef;
    DevBuf dscan, ditems, dwin, dlohi, dmom, dpart, dsums, dfreq, dcols, dempty;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    const int64_t ncols = Nf * nwin * ns;
    LPVS_TRY(dpower.set(power, average ? Nf * ns : ncols));
    if (coef) LPVS_TRY(dcoef.set(coef, 3 * ncols));
    // the record is held to g4's rules as a whole: a non-finite t, y or W, a negative weight (the scan's sum of W is not used, and the
    // small record has no means or moments: every window has its own).  Its tail: the degenerate count
    LPVS_TRY(rec.alloc_small(1, false));
    unsigned long long *ndeg_dev = rec.tail<unsigned long long>();
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)lomb_sum_slabs(N)));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    // the work list and the windows: [starts | counts | offset] (int64), nslab (int32) behind them; [lo | hi]
    LPVS_TRY(ditems.alloc(sizeof(LombWindowItem) * (size_t)nitems));
    LPVS_TRY(copy_to_device(ditems.p, plan.items.data(), sizeof(LombWindowItem) * (size_t)nitems, s));
    LPVS_TRY(dwin.alloc(sizeof(int64_t) * (size_t)(3 * nwin) + sizeof(int32_t) * (size_t)nwin));
    int64_t *starts_dev = dwin.as<int64_t>(), *counts_dev = starts_dev + nwin, *offset_dev = counts_dev + nwin;
    int32_t *nslab_dev = reinterpret_cast<int32_t *>(offset_dev + nwin);
    LPVS_TRY(copy_to_device(starts_dev, starts.data(), sizeof(int64_t) * (size_t)nwin, s));
    LPVS_TRY(copy_to_device(counts_dev, counts.data(), sizeof(int64_t) * (size_t)nwin, s));
    LPVS_TRY(copy_to_device(offset_dev, plan.offset.data(), sizeof(int64_t) * (size_t)nwin, s));
    LPVS_TRY(copy_to_device(nslab_dev, plan.nslab.data(), sizeof(int32_t) * (size_t)nwin, s));
    LPVS_TRY(dlohi.alloc(sizeof(double) * (size_t)(2 * nwin)));
    LPVS_TRY(copy_to_device(dlohi.p, lo, sizeof(double) * (size_t)nwin, s));
    LPVS_TRY(copy_to_device(dlohi.as<double>() + nwin, hi, sizeof(double) * (size_t)nwin, s));
    LombWindows A;
    A.t = rec.t.p; A.y = rec.y.p; A.W = rec.W.p; A.N = N; A.nwin = nwin; A.nitems = nitems; A.ns = (int)ns; A.taper = taper;
    A.items = ditems.as<LombWindowItem>(); A.starts = starts_dev; A.counts = counts_dev; A.offset = offset_dev; A.nslab = nslab_dev;
    A.lo = dlohi.as<double>(); A.hi = A.lo + nwin;
    // per window: [0] sum W g, [1 .. ns] the weighted means, then Y_c, YY_c per signal and sum w y_c^2 of the signals as given
    LPVS_TRY(dmom.alloc(sizeof(double) * (size_t)(nwin * (1 + 4 * ns))));
    double *swg_dev = dmom.as<double>(), *mean_dev = swg_dev + nwin, *mom_dev = mean_dev + nwin * ns;
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)(nitems * nrow * Nf > 3 * ns * nitems ? nitems * nrow * Nf : 3 * ns * nitems)));
    LPVS_TRY(launch_lomb_windows_moments(A, center, swg_dev, mean_dev, mom_dev, dpart.as<double>(), s));
    LPVS_TRY(dsums.alloc(sizeof(double) * (size_t)(nwin * nrow * Nf)));
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, hf.data(), sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(clock.mark(1));
    LPVS_TRY(launch_lomb_windows_direct(A, dfreq.as<double>(), Nf, tl, swg_dev, center ? mean_dev : nullptr, dpart.as<double>(), dsums.as<double>(), s));
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(dempty.alloc(sizeof(int32_t) * (size_t)nwin));
    double *cols = dpower.p;
    if (average) { LPVS_TRY(dcols.alloc(sizeof(double) * (size_t)ncols)); cols = dcols.as<double>(); }
    LPVS_TRY(launch_lomb_windows_epilogue(A, dsums.as<double>(), Nf, swg_dev, mom_dev, mean_dev, fit_mean, center, psd, cols, coef ? dcoef.p : nullptr,
                                          dempty.as<int32_t>(), rec.flags_dev, ndeg_dev, s));
    if (average) LPVS_TRY(launch_lomb_windows_average(cols, Nf, nwin, ns, dempty.as<int32_t>(), dpower.p, s));
    LPVS_TRY(clock.mark(3));
    unsigned long long ndeg = 0;
    LPVS_TRY(rec.check("lombscargle", WeightSum::unused));                // (only now: one read-back answers for the scan and the epilogue)
    if (rec.flags & 4) { set_error("lombscargle: the weights of a window do not sum to a finite value"); return LPVS_EARGUMENT; }
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(ndeg), s));
    std::vector<int32_t> hempty((size_t)nwin);
    LPVS_TRY(copy_from_device(hempty.data(), dempty.p, sizeof(int32_t) * (size_t)nwin, s));
    int64_t nempty = 0;
    for (int64_t w = 0; w < nwin; ++w) { nempty += hempty[(size_t)w]; if (empty_out) empty_out[w] = hempty[(size_t)w]; }
    LPVS_TRY(dpower.finish(s));
    if (coef) LPVS_TRY(dcoef.finish(s));
    LPVS_TRY(clock.finish());
    double *g = g_lomb_windows_timing;
    g[0] = (double)nwin; g[1] = (double)nempty; g[2] = (double)nitems; g[3] = (double)plan.slab_samples; g[4] = (double)ndeg;
    for (int i = 0; i < 4; ++i) g[5 + i] = clock.ms(i);
    g[9] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_lombscargle_windows_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, const int64_t *starts,
                                     const int64_t *counts, const double *lo, const double *hi, int64_t nwin, int32_t taper, int32_t fit_mean, int32_t center_data,
                                     int32_t normalization, int32_t average, int32_t device, double *power, double *coef, int32_t *empty_out) {
    try {
        if (!y || !t || !f || !power || !starts || !counts || !lo || !hi) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (N <= 0 || Nf <= 0 || ns <= 0 || ns > 65535 || nwin <= 0) {
            set_error("need N > 0, Nf > 0, nwin > 0 and 1 <= ns <= 65535 (N = %lld, Nf = %lld, nwin = %lld, ns = %lld)", (long long)N, (long long)Nf, (long long)nwin, (long long)ns);
            return LPVS_EARGUMENT;
        }
        if (Nf > ((int64_t)1 << 24)) { set_error("%lld frequencies are too many", (long long)Nf); return LPVS_EUNSUPPORTED; }
        if (nwin > kLombMaxWindows) { set_error("lombscargle: %lld windows are more than 2^24", (long long)nwin); return LPVS_EUNSUPPORTED; }
        if (taper != LPVS_TAPER_RECT && taper != LPVS_TAPER_HANN) { set_error("taper must be 0 (rect) or 1 (hann), got %d", taper); return LPVS_EARGUMENT; }
        LPVS_TRY(check_normalization(normalization));
        if (average && coef) { set_error("lombscargle: the coefficients of an average over windows are not defined (coef with average)"); return LPVS_EARGUMENT; }
        if (is_device_ptr(f) || is_device_ptr(starts) || is_device_ptr(counts) || is_device_ptr(lo) || is_device_ptr(hi) || (empty_out && is_device_ptr(empty_out))) {
            set_error("lombscargle: f, starts, counts, lo, hi and empty_out are host memory"); return LPVS_EARGUMENT;
        }
        std::vector<double> hf;
        LPVS_TRY(host_frequencies(f, Nf, hf));
        std::vector<int64_t> hs(starts, starts + nwin), hc(counts, counts + nwin);
        for (int64_t w = 0; w < nwin; ++w) {
            if (hs[(size_t)w] < 0 || hc[(size_t)w] < 0 || hs[(size_t)w] > N || hc[(size_t)w] > N - hs[(size_t)w]) {
                set_error("lombscargle: window %lld covers the samples [%lld, %lld + %lld), outside [0, %lld]", (long long)w, (long long)hs[(size_t)w],
                          (long long)hs[(size_t)w], (long long)hc[(size_t)w], (long long)N);
                return LPVS_EARGUMENT;
            }
            if (!std::isfinite(lo[w]) || !std::isfinite(hi[w])) { set_error("lombscargle: the time interval of window %lld is not finite", (long long)w); return LPVS_EARGUMENT; }
            if (hi[w] < lo[w]) { set_error("lombscargle: the time interval of window %lld ends before it begins", (long long)w); return LPVS_EARGUMENT; }
        }
        return lomb_windows_impl(y, ns, t, N, W, hf, hs, hc, lo, hi, taper, fit_mean != 0, center_data != 0, normalization == LPVS_LOMB_PSD, average != 0, device,
                                 power, coef, empty_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_lombscargle_windows_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_lomb_windows_timing, 10);
}

int32_t lpvs_time_windows_f64(const double *t, int64_t N, const double *lo, const double *hi, int64_t nwin, int32_t device, int64_t *starts_out,
                              int64_t *counts_out) {
    try {
        if (!t || !lo || !hi || !starts_out || !counts_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (N <= 0 || nwin <= 0 || nwin > kLombMaxWindows) { set_error("time_windows: need N > 0 and 1 <= nwin <= 2^24 (N = %lld, nwin = %lld)", (long long)N, (long long)nwin); return LPVS_EARGUMENT; }
        if (is_device_ptr(lo) || is_device_ptr(hi) || is_device_ptr(starts_out) || is_device_ptr(counts_out)) {
            set_error("time_windows: lo, hi, starts_out and counts_out are host memory"); return LPVS_EARGUMENT;
        }
        for (int64_t w = 0; w < nwin; ++w)
            if (!std::isfinite(lo[w]) || !std::isfinite(hi[w])) { set_error("time_windows: the time interval of window %lld is not finite", (long long)w); return LPVS_EARGUMENT; }
        LPVS_TRY(Record::admit(device));
        hipStream_t s = nullptr;
        Staged<double> dt; DevBuf dlohi, dedges, dflags;
        DrainOnExit drain(s);
        LPVS_TRY(dt.set(t, N, device, s));
        LPVS_TRY(dlohi.alloc(sizeof(double) * (size_t)(2 * nwin)));
        LPVS_TRY(copy_to_device(dlohi.p, lo, sizeof(double) * (size_t)nwin, s));
        LPVS_TRY(copy_to_device(dlohi.as<double>() + nwin, hi, sizeof(double) * (size_t)nwin, s));
        LPVS_TRY(dedges.alloc(sizeof(int64_t) * (size_t)(2 * nwin)));
        LPVS_TRY(dflags.alloc(sizeof(int)));
        LPVS_TRY(launch_lomb_time_windows(dt.p, N, dlohi.as<double>(), dlohi.as<double>() + nwin, nwin, dflags.as<int>(), dedges.as<int64_t>(), s));
        int flags = 0;
        LPVS_TRY(copy_from_device(&flags, dflags.p, sizeof(int), s));
        if (flags & 1) { set_error("time_windows: t holds a value that is not finite"); return LPVS_EARGUMENT; }
        if (flags & 8) { set_error("time_windows: t is not sorted (it decreases somewhere)"); return LPVS_EARGUMENT; }
        std::vector<int64_t> edges((size_t)(2 * nwin));
        LPVS_TRY(copy_from_device(edges.data(), dedges.p, sizeof(int64_t) * edges.size(), s));
        for (int64_t w = 0; w < nwin; ++w) {
            const int64_t a = edges[(size_t)(2 * w)], b = edges[(size_t)(2 * w + 1)];
            starts_out[w] = a; counts_out[w] = b > a ? b - a : 0;
        }
        return LPVS_OK;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

// ---- weighted wavelet Z-transform (wwz.hip; the decisions: wwz_plan.h) ------------------------------------------------------------------------
// what lpvs_wwz_last_timing reports of the calling thread's last call: [0] Nf, [1] Ntau, [2] times and [3] signals per thread of the sums
// kernel, [4] work items, [5] slab length, [6] empty cells, [7] degenerate cells, [8] staged and [9] useful (sample, frequency, time)
// triples, ms of [10] staging, the scan and the record's means, [11] the ranges and the work list, [12] the sums, [13] the epilogue,
// [14] the copy-out, [15] total
static thread_local double g_wwz_timing[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t wwz_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, const double *tau, int64_t Ntau,
                        const double *radius, const WwzShape &sh, bool center, int32_t device, double *power, double *amplitude, double *wwz, double *neff,
                        double *coef, int64_t *count_out, int32_t *empty_out) {
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<6> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dpower, damp, dwwz, dneff, dcoef;
    DevBuf dscan, dfreq, dtau, dpos, dedges, dpair, ditems, dlist, dpart, dcount, dempty;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    const int64_t cells = Nf * Ntau, ncols = cells * ns, pairs = sh.ngroups * sh.ftiles;
    LPVS_TRY(dpower.set(power, ncols));
    LPVS_TRY(damp.set(amplitude, ncols));
    LPVS_TRY(dwwz.set(wwz, ncols));
    LPVS_TRY(dneff.set(neff, cells));
    if (coef) LPVS_TRY(dcoef.set(coef, 3 * ncols));
    // the small record (its moments are not used); its tail: the two counters of the epilogue
    LPVS_TRY(rec.alloc_small(2));
    unsigned long long *counters_dev = rec.tail<unsigned long long>();
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    LPVS_TRY(launch_wwz_sorted(rec.t.p, N, rec.flags_dev, s));
    LPVS_TRY(rec.check("wwz", WeightSum::finite));
    // the record's weighted means (weights W); weights that sum to 0 leave every cell empty, and nothing is removed
    const bool removes = center && rec.sumW > 0.0;
    if (removes) LPVS_TRY(rec.moments(true, dscan.as<double>()));
    LPVS_TRY(clock.mark(1));
    // per frequency [f | decay | radius | rmax of the tiles], per time [tau in order | gmin | gmax | tau as given], the places
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)(3 * Nf + sh.ftiles)));
    double *f_dev = dfreq.as<double>(), *decay_dev = f_dev + Nf, *radius_dev = decay_dev + Nf, *rmax_dev = radius_dev + Nf;
    LPVS_TRY(copy_to_device(f_dev, f, sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(copy_to_device(decay_dev, sh.decay.data(), sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(copy_to_device(radius_dev, radius, sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(copy_to_device(rmax_dev, sh.rmax.data(), sizeof(double) * (size_t)sh.ftiles, s));
    const int64_t nsorted = sh.ngroups * sh.TT;
    LPVS_TRY(dtau.alloc(sizeof(double) * (size_t)(nsorted + 2 * sh.ngroups + Ntau)));
    double *tau_dev = dtau.as<double>(), *gmin_dev = tau_dev + nsorted, *gmax_dev = gmin_dev + sh.ngroups, *given_dev = gmax_dev + sh.ngroups;
    LPVS_TRY(copy_to_device(tau_dev, sh.tau_sorted.data(), sizeof(double) * (size_t)nsorted, s));
    LPVS_TRY(copy_to_device(gmin_dev, sh.gmin.data(), sizeof(double) * (size_t)sh.ngroups, s));
    LPVS_TRY(copy_to_device(gmax_dev, sh.gmax.data(), sizeof(double) * (size_t)sh.ngroups, s));
    LPVS_TRY(copy_to_device(given_dev, tau, sizeof(double) * (size_t)Ntau, s));
    LPVS_TRY(dpos.alloc(sizeof(int32_t) * (size_t)Ntau));
    LPVS_TRY(copy_to_device(dpos.p, sh.pos.data(), sizeof(int32_t) * (size_t)Ntau, s));
    // the ranges of the cells and of the (group, tile) pairs; the pairs' go to the host, which lays out the work list
    LPVS_TRY(dedges.alloc(sizeof(int64_t) * (size_t)(2 * cells)));
    LPVS_TRY(dpair.alloc(sizeof(int64_t) * (size_t)(2 * pairs)));
    LPVS_TRY(launch_wwz_ranges(rec.t.p, N, given_dev, given_dev, Ntau, radius_dev, Nf, dedges.as<int64_t>(), s));
    LPVS_TRY(launch_wwz_ranges(rec.t.p, N, gmin_dev, gmax_dev, sh.ngroups, rmax_dev, sh.ftiles, dpair.as<int64_t>(), s));
    std::vector<int64_t> hedges((size_t)(2 * cells)), hpair((size_t)(2 * pairs));
    LPVS_TRY(copy_from_device(hedges.data(), dedges.p, sizeof(int64_t) * hedges.size(), s));
    LPVS_TRY(copy_from_device(hpair.data(), dpair.p, sizeof(int64_t) * hpair.size(), s));
    double useful = 0;
    for (int64_t q = 0; q < cells; ++q) {
        const int64_t a = hedges[(size_t)(2 * q)], b = hedges[(size_t)(2 * q + 1)];
        if (b > a) useful += (double)(b - a);
    }
    const WwzWork work = wwz_work(sh, hpair, useful);
    if (work.status != kWwzOk) { set_error("%s", work.why.c_str()); return LPVS_EUNSUPPORTED; }
    const int64_t nitems = (int64_t)work.items.size();
    LPVS_TRY(ditems.alloc(sizeof(WwzItem) * (size_t)(nitems > 0 ? nitems : 1)));
    if (nitems > 0) LPVS_TRY(copy_to_device(ditems.p, work.items.data(), sizeof(WwzItem) * (size_t)nitems, s));
    LPVS_TRY(dlist.alloc(sizeof(int64_t) * (size_t)(2 * pairs + 1)));
    int64_t *offset_dev = dlist.as<int64_t>(), *first_slab_dev = offset_dev + pairs + 1;
    LPVS_TRY(copy_to_device(offset_dev, work.offset.data(), sizeof(int64_t) * (size_t)(pairs + 1), s));
    LPVS_TRY(copy_to_device(first_slab_dev, work.first_slab.data(), sizeof(int64_t) * (size_t)pairs, s));
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)(work.part_doubles > 0 ? work.part_doubles : 1)));
    WwzArgs A;
    A.t = rec.t.p; A.y = rec.y.p; A.W = rec.W.p; A.mean = removes ? rec.mean_dev : nullptr;
    A.f = f_dev; A.decay = decay_dev; A.radius = radius_dev; A.tau = tau_dev; A.pos = dpos.as<int32_t>();
    A.items = ditems.as<WwzItem>(); A.offset = offset_dev; A.first_slab = first_slab_dev;
    A.N = N; A.Nf = Nf; A.Ntau = Ntau; A.nitems = nitems; A.ftiles = sh.ftiles; A.slab_samples = sh.slab_samples; A.rows = sh.rows;
    A.ns = (int)ns; A.TT = sh.TT;
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_wwz_sums(A, sh.ts, dpart.as<double>(), s));
    LPVS_TRY(clock.mark(3));
    LPVS_TRY(dcount.alloc(sizeof(int64_t) * (size_t)cells));
    LPVS_TRY(dempty.alloc(sizeof(int32_t) * (size_t)cells));
    LPVS_TRY(launch_wwz_epilogue(A, dpart.as<double>(), dedges.as<int64_t>(), removes, dpower.p, damp.p, dwwz.p, dneff.p, coef ? dcoef.p : nullptr,
                                 dcount.as<int64_t>(), dempty.as<int32_t>(), rec.flags_dev, counters_dev, s));
    LPVS_TRY(clock.mark(4));
    unsigned long long counters[2] = {0, 0};
    int flags = 0;                                                        // (what the epilogue added to them)
    LPVS_TRY(copy_from_device(&flags, rec.flags_dev, sizeof(int), s));
    LPVS_TRY(copy_from_device(counters, counters_dev, sizeof(counters), s));
    if (flags & 4) { set_error("wwz: the weights of a cell do not sum to a finite value"); return LPVS_EARGUMENT; }
    if (flags & 16) { set_error("wwz: a cell lies outside the samples its group stages"); return LPVS_EDEVICE; }
    if (count_out) LPVS_TRY(copy_from_device(count_out, dcount.p, sizeof(int64_t) * (size_t)cells, s));
    if (empty_out) LPVS_TRY(copy_from_device(empty_out, dempty.p, sizeof(int32_t) * (size_t)cells, s));
    LPVS_TRY(dpower.finish(s));
    LPVS_TRY(damp.finish(s));
    LPVS_TRY(dwwz.finish(s));
    LPVS_TRY(dneff.finish(s));
    if (coef) LPVS_TRY(dcoef.finish(s));
    LPVS_TRY(clock.finish());
    double *g = g_wwz_timing;
    g[0] = (double)Nf; g[1] = (double)Ntau; g[2] = sh.TT; g[3] = sh.ts; g[4] = (double)nitems; g[5] = (double)sh.slab_samples;
    g[6] = (double)counters[0]; g[7] = (double)counters[1]; g[8] = work.staged; g[9] = work.useful;
    for (int i = 0; i < 5; ++i) g[10 + i] = clock.ms(i);
    g[15] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_wwz_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, const double *tau, int64_t Ntau,
                     double c, const double *radius, int32_t center_data, int32_t device, double *power_out, double *amplitude_out, double *wwz_out,
                     double *neff_out, double *coef_out, int64_t *count_out, int32_t *empty_out) {
    try {
        if (!y || !t || !f || !tau || !radius || !power_out || !amplitude_out || !wwz_out || !neff_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (is_device_ptr(f) || is_device_ptr(tau) || is_device_ptr(radius) || (count_out && is_device_ptr(count_out)) || (empty_out && is_device_ptr(empty_out))) {
            set_error("wwz: f, tau, radius, count_out and empty_out are host memory"); return LPVS_EARGUMENT;
        }
        const WwzShape sh = wwz_shape(N, ns, f, Nf, tau, Ntau, c, radius);        // (the counts are checked before an array is read)
        if (sh.status != kWwzOk) { set_error("%s", sh.why.c_str()); return sh.status == kWwzArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        return wwz_impl(y, ns, t, N, W, f, Nf, tau, Ntau, radius, sh, center_data != 0, device, power_out, amplitude_out, wwz_out, neff_out, coef_out, count_out,
                        empty_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_wwz_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_wwz_timing, 16);
}

// ---- box least squares periodogram (bls.hip; the decisions: bls_plan.h) ------------------------------------------------------------------------
// what lpvs_bls_last_timing reports of the calling thread's last call: [0] frequencies per workgroup (F), [1] signals per pass (TS),
// [2] passes, [3] LDS bytes of a workgroup, [4] the shift of the weights (60; 0 with unit weights: counts), [5], [6] the smallest and
// largest shift of a signal (0, 0 when every signal is constant), [7] degenerate (frequency, signal) pairs, [8] boxes tried (per signal),
// [9] unit weights, ms of [10] staging, the scan and the moments, [11] the maxima and the quantisation, [12] fold and search,
// [13] the copy-out, [14] total, [15] Nf
static thread_local double g_bls_timing[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t bls_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nbins, const int32_t *kmin,
                        const int32_t *kmax, int64_t min_count, bool dips_only, bool center, bool chi2, const BlsPlan &plan, int32_t device, double *power,
                        double *depth, double *depth_err, int32_t *start_out, int32_t *width_out, int64_t *count_out, int32_t *degenerate_out, int64_t *hist_out,
                        int32_t *hcount_out) {
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dpower, ddepth, derr;
    DevBuf dscan, dq, dfreq, dk, dshy, dint, dcount, dhist, dhcount;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    const int64_t ncols = Nf * ns;
    LPVS_TRY(dpower.set(power, ncols));
    LPVS_TRY(ddepth.set(depth, ncols));
    LPVS_TRY(derr.set(depth_err, ncols));
    // the tail of the small record: the maxima (2 ns), the two words of every YY (2 ns), the degenerate counter
    LPVS_TRY(rec.alloc_small((size_t)(4 * ns) + 1));
    unsigned long long *amax_dev = rec.tail<unsigned long long>();
    long long *yyacc_dev = reinterpret_cast<long long *>(amax_dev + 2 * ns);
    unsigned long long *ndeg_dev = amax_dev + 4 * ns;
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    LPVS_TRY(rec.check("bls", WeightSum::positive));
    LPVS_TRY(rec.moments(center, dscan.as<double>()));
    LPVS_TRY(clock.mark(1));
    // the maxima, the shifts (bls_plan.h), the quantised record: qy[ns][N], then qw[N] with weights
    LPVS_TRY(launch_bls_max(rec.y.p, rec.wy.as<double>(), rec.mean_dev, center, N, ns, amax_dev, s));
    std::vector<unsigned long long> hmax((size_t)(2 * ns));
    LPVS_TRY(copy_from_device(hmax.data(), amax_dev, sizeof(unsigned long long) * (size_t)(2 * ns), s));
    std::vector<int32_t> hshy((size_t)(2 * ns), 0);
    int shy_lo = 0, shy_hi = 0; bool any = false;
    for (int64_t c = 0; c < ns; ++c) {
        double A, M;
        memcpy(&A, &hmax[(size_t)c], sizeof(double)); memcpy(&M, &hmax[(size_t)(ns + c)], sizeof(double));
        hshy[(size_t)(ns + c)] = M > 0.0 && std::isfinite(M) ? bls_shift_y(M, N) : kBlsNoShift;   // (the terms of YY_c: cut against the largest)
        if (!(A > 0.0)) continue;
        const int sh = bls_shift_y(A, N);
        hshy[(size_t)c] = sh;
        shy_lo = any && shy_lo < sh ? shy_lo : sh;
        shy_hi = any && shy_hi > sh ? shy_hi : sh;
        any = true;
    }
    LPVS_TRY(dshy.alloc(sizeof(int32_t) * (size_t)(2 * ns)));
    LPVS_TRY(copy_to_device(dshy.p, hshy.data(), sizeof(int32_t) * (size_t)(2 * ns), s));
    LPVS_TRY(dq.alloc(sizeof(long long) * (size_t)(N * (ns + (plan.unit ? 0 : 1)))));
    long long *qy_dev = dq.as<long long>(), *qw_dev = plan.unit ? nullptr : qy_dev + N * ns;
    LPVS_TRY(launch_bls_quantise(rec.y.p, rec.w.as<double>(), rec.wy.as<double>(), rec.mean_dev, center, N, ns, plan.log2n, dshy.as<int32_t>(), amax_dev, qw_dev, qy_dev, yyacc_dev, s));
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, f, sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(dk.alloc(sizeof(int32_t) * (size_t)(2 * Nf)));
    LPVS_TRY(copy_to_device(dk.p, kmin, sizeof(int32_t) * (size_t)Nf, s));
    LPVS_TRY(copy_to_device(dk.as<int32_t>() + Nf, kmax, sizeof(int32_t) * (size_t)Nf, s));
    LPVS_TRY(dint.alloc(sizeof(int32_t) * (size_t)(3 * ncols)));
    LPVS_TRY(dcount.alloc(sizeof(int64_t) * (size_t)ncols));
    if (hist_out) LPVS_TRY(dhist.alloc(sizeof(int64_t) * (size_t)(Nf * (1 + ns) * nbins)));
    if (hcount_out) LPVS_TRY(dhcount.alloc(sizeof(int32_t) * (size_t)(Nf * nbins)));
    BlsArgs A;
    A.t = rec.t.p; A.qw = qw_dev; A.qy = qy_dev; A.f = dfreq.as<double>(); A.kmin = dk.as<int32_t>(); A.kmax = A.kmin + Nf;
    A.shy = dshy.as<int32_t>(); A.amax = amax_dev; A.yyacc = yyacc_dev; A.mom = rec.mom_dev; A.log2n = plan.log2n;
    A.N = N; A.Nf = Nf; A.min_count = min_count; A.ns = (int)ns; A.nbins = nbins; A.dips_only = dips_only ? 1 : 0; A.chi2 = chi2 ? 1 : 0;
    A.center = center ? 1 : 0; A.sumW = rec.sumW;
    A.power = dpower.p; A.depth = ddepth.p; A.depth_err = derr.p;
    A.start = dint.as<int32_t>(); A.width = A.start + ncols; A.degenerate = A.width + ncols; A.count = dcount.as<int64_t>();
    A.hist = hist_out ? dhist.as<long long>() : nullptr; A.hcount = hcount_out ? dhcount.as<int32_t>() : nullptr; A.ndeg = ndeg_dev;
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_bls(A, plan, s));
    LPVS_TRY(clock.mark(3));
    unsigned long long ndeg = 0;
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(ndeg), s));
    LPVS_TRY(copy_from_device(start_out, A.start, sizeof(int32_t) * (size_t)ncols, s));
    LPVS_TRY(copy_from_device(width_out, A.width, sizeof(int32_t) * (size_t)ncols, s));
    LPVS_TRY(copy_from_device(count_out, A.count, sizeof(int64_t) * (size_t)ncols, s));
    if (degenerate_out) LPVS_TRY(copy_from_device(degenerate_out, A.degenerate, sizeof(int32_t) * (size_t)ncols, s));
    if (hist_out) LPVS_TRY(copy_from_device(hist_out, dhist.p, sizeof(int64_t) * (size_t)(Nf * (1 + ns) * nbins), s));
    if (hcount_out) LPVS_TRY(copy_from_device(hcount_out, dhcount.p, sizeof(int32_t) * (size_t)(Nf * nbins), s));
    LPVS_TRY(dpower.finish(s));
    LPVS_TRY(ddepth.finish(s));
    LPVS_TRY(derr.finish(s));
    LPVS_TRY(clock.finish());
    double *g = g_bls_timing;
    g[0] = plan.F; g[1] = plan.ts; g[2] = plan.passes; g[3] = (double)plan.lds_bytes; g[4] = plan.unit ? 0 : kBlsWeightShift; g[5] = shy_lo; g[6] = shy_hi;
    g[7] = (double)ndeg; g[8] = plan.boxes; g[9] = plan.unit; g[15] = (double)Nf;
    for (int i = 0; i < 4; ++i) g[10 + i] = clock.ms(i);
    g[14] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_bls_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nbins, const int32_t *kmin,
                     const int32_t *kmax, int64_t min_count, int32_t dips_only, int32_t center_data, int32_t normalization, int32_t device, double *power_out,
                     double *depth_out, double *depth_err_out, int32_t *start_out, int32_t *width_out, int64_t *count_out, int32_t *degenerate_out, int64_t *hist_out,
                     int32_t *hcount_out) {
    try {
        if (!y || !t || !f || !kmin || !kmax || !power_out || !depth_out || !depth_err_out || !start_out || !width_out || !count_out) {
            set_error("NULL argument"); return LPVS_EARGUMENT;
        }
        if (is_device_ptr(f) || is_device_ptr(kmin) || is_device_ptr(kmax) || is_device_ptr(start_out) || is_device_ptr(width_out) || is_device_ptr(count_out) ||
            (degenerate_out && is_device_ptr(degenerate_out)) || (hist_out && is_device_ptr(hist_out)) || (hcount_out && is_device_ptr(hcount_out))) {
            set_error("bls: f, kmin, kmax, start_out, width_out, count_out, degenerate_out, hist_out and hcount_out are host memory"); return LPVS_EARGUMENT;
        }
        const BlsPlan plan = bls_plan(N, ns, f, Nf, nbins, kmin, kmax, min_count, W == nullptr, normalization);   // (the counts are checked before an array is read)
        if (plan.status != kBlsOk) { set_error("%s", plan.why.c_str()); return plan.status == kBlsArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        return bls_impl(y, ns, t, N, W, f, Nf, nbins, kmin, kmax, min_count, dips_only != 0, center_data != 0, normalization == 1, plan, device, power_out, depth_out,
                        depth_err_out, start_out, width_out, count_out, degenerate_out, hist_out, hcount_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_bls_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_bls_timing, 16);
}

// ---- fold statistics: pdm / aov and the conditional entropy (fold.hip; the decisions: fold_plan.h) ------------------------------------------------
// what lpvs_pdm_last_timing reports of the calling thread's last call: [0] frequencies per workgroup (F), [1] signals per pass (TS),
// [2] passes, [3] LDS bytes of a workgroup, [4] copies (1: pdm keeps one histogram), [5] the shift of the weights (60; 0 with unit
// weights), [6], [7] the smallest and largest shift of a signal (0, 0 when every signal is constant), [8] degenerate (frequency, signal)
// pairs, [9] unit weights, ms of [10] staging, the scan and the moments, [11] the maxima and the quantisation, [12] fold and pooling,
// [13] the copy-out, [14] total, [15] Nf
static thread_local double g_pdm_timing[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t pdm_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t covers, bool center,
                        const PdmPlan &plan, int32_t device, double *explained, int32_t *nonempty_out, int32_t *degenerate_out, int64_t *hist_out,
                        int32_t *hcount_out) {
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dexp;
    DevBuf dscan, dq, dfreq, dshy, dint, dhist, dhcount;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
    const int64_t ncols = Nf * ns, nfine = plan.nfine;
    LPVS_TRY(dexp.set(explained, ncols));
    // the tail of the small record: the maxima (2 ns), the two words of every YY (2 ns), the degenerate counter
    LPVS_TRY(rec.alloc_small((size_t)(4 * ns) + 1));
    unsigned long long *amax_dev = rec.tail<unsigned long long>();
    long long *yyacc_dev = reinterpret_cast<long long *>(amax_dev + 2 * ns);
    unsigned long long *ndeg_dev = amax_dev + 4 * ns;
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    LPVS_TRY(rec.check("pdm", WeightSum::positive));
    LPVS_TRY(rec.moments(center, dscan.as<double>()));
    LPVS_TRY(clock.mark(1));
    // the maxima, the shifts (bls_plan.h), the quantised record: qy[ns][N], then qw[N] with weights
    LPVS_TRY(launch_bls_max(rec.y.p, rec.wy.as<double>(), rec.mean_dev, center, N, ns, amax_dev, s));
    std::vector<unsigned long long> hmax((size_t)(2 * ns));
    LPVS_TRY(copy_from_device(hmax.data(), amax_dev, sizeof(unsigned long long) * (size_t)(2 * ns), s));
    std::vector<int32_t> hshy((size_t)(2 * ns), 0);
    int shy_lo = 0, shy_hi = 0; bool any = false;
    for (int64_t c = 0; c < ns; ++c) {
        double A, M;
        memcpy(&A, &hmax[(size_t)c], sizeof(double)); memcpy(&M, &hmax[(size_t)(ns + c)], sizeof(double));
        hshy[(size_t)(ns + c)] = M > 0.0 && std::isfinite(M) ? bls_shift_y(M, N) : kBlsNoShift;
        if (!(A > 0.0)) continue;
        const int sh = bls_shift_y(A, N);
        hshy[(size_t)c] = sh;
        shy_lo = any && shy_lo < sh ? shy_lo : sh;
        shy_hi = any && shy_hi > sh ? shy_hi : sh;
        any = true;
    }
    LPVS_TRY(dshy.alloc(sizeof(int32_t) * (size_t)(2 * ns)));
    LPVS_TRY(copy_to_device(dshy.p, hshy.data(), sizeof(int32_t) * (size_t)(2 * ns), s));
    LPVS_TRY(dq.alloc(sizeof(long long) * (size_t)(N * (ns + (plan.unit ? 0 : 1)))));
    long long *qy_dev = dq.as<long long>(), *qw_dev = plan.unit ? nullptr : qy_dev + N * ns;
    LPVS_TRY(launch_bls_quantise(rec.y.p, rec.w.as<double>(), rec.wy.as<double>(), rec.mean_dev, center, N, ns, plan.log2n, dshy.as<int32_t>(), amax_dev, qw_dev, qy_dev, yyacc_dev, s));
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, f, sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(dint.alloc(sizeof(int32_t) * (size_t)(ncols + Nf)));
    if (hist_out) LPVS_TRY(dhist.alloc(sizeof(int64_t) * (size_t)(Nf * (1 + ns) * nfine)));
    if (hcount_out) LPVS_TRY(dhcount.alloc(sizeof(int32_t) * (size_t)(Nf * nfine)));
    PdmArgs A;
    A.t = rec.t.p; A.qw = qw_dev; A.qy = qy_dev; A.f = dfreq.as<double>();
    A.shy = dshy.as<int32_t>(); A.amax = amax_dev; A.yyacc = yyacc_dev; A.mom = rec.mom_dev; A.log2n = plan.log2n;
    A.N = N; A.Nf = Nf; A.ns = (int)ns; A.nfine = plan.nfine; A.covers = covers; A.center = center ? 1 : 0;
    A.explained = dexp.p; A.degenerate = dint.as<int32_t>(); A.nonempty = A.degenerate + ncols;
    A.hist = hist_out ? dhist.as<long long>() : nullptr; A.hcount = hcount_out ? dhcount.as<int32_t>() : nullptr; A.ndeg = ndeg_dev;
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_pdm(A, plan, s));
    LPVS_TRY(clock.mark(3));
    unsigned long long ndeg = 0;
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(ndeg), s));
    LPVS_TRY(copy_from_device(nonempty_out, A.nonempty, sizeof(int32_t) * (size_t)Nf, s));
    LPVS_TRY(copy_from_device(degenerate_out, A.degenerate, sizeof(int32_t) * (size_t)ncols, s));
    if (hist_out) LPVS_TRY(copy_from_device(hist_out, dhist.p, sizeof(int64_t) * (size_t)(Nf * (1 + ns) * nfine), s));
    if (hcount_out) LPVS_TRY(copy_from_device(hcount_out, dhcount.p, sizeof(int32_t) * (size_t)(Nf * nfine), s));
    LPVS_TRY(dexp.finish(s));
    LPVS_TRY(clock.finish());
    double *g = g_pdm_timing;
    g[0] = plan.F; g[1] = plan.ts; g[2] = plan.passes; g[3] = (double)plan.lds_bytes; g[4] = 1; g[5] = plan.unit ? 0 : kBlsWeightShift; g[6] = shy_lo; g[7] = shy_hi;
    g[8] = (double)ndeg; g[9] = plan.unit; g[15] = (double)Nf;
    for (int i = 0; i < 4; ++i) g[10 + i] = clock.ms(i);
    g[14] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_pdm_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int32_t nbins, int32_t covers,
                     int32_t center_data, int32_t device, double *explained_out, int32_t *nonempty_out, int32_t *degenerate_out, int64_t *hist_out,
                     int32_t *hcount_out) {
    try {
        if (!y || !t || !f || !explained_out || !nonempty_out || !degenerate_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (is_device_ptr(f) || is_device_ptr(nonempty_out) || is_device_ptr(degenerate_out) || (hist_out && is_device_ptr(hist_out)) ||
            (hcount_out && is_device_ptr(hcount_out))) {
            set_error("pdm: f, nonempty_out, degenerate_out, hist_out and hcount_out are host memory"); return LPVS_EARGUMENT;
        }
        const PdmPlan plan = pdm_plan(N, ns, f, Nf, nbins, covers, W == nullptr);   // (the counts are checked before an array is read)
        if (plan.status != kFoldOk) { set_error("%s", plan.why.c_str()); return plan.status == kFoldArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        return pdm_impl(y, ns, t, N, W, f, Nf, covers, center_data != 0, plan, device, explained_out, nonempty_out, degenerate_out, hist_out, hcount_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_pdm_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_pdm_timing, 16);
}

// what lpvs_cent_last_timing reports of the calling thread's last call: [0] F, [1] TS, [2] passes, [3] LDS bytes of a workgroup, [4] copies
// of the count histogram, [5], [6], [7] 0 (nothing is quantised: no shifts), [8] degenerate signals, [9] 1 (unweighted), ms of
// [10] staging and the scan, [11] the extremes and the value bins, [12] fold and entropy, [13] the copy-out, [14] total, [15] Nf
static thread_local double g_cent_timing[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t cent_impl(const double *y, int64_t ns, const double *t, int64_t N, const double *f, int64_t Nf, int32_t nbins, int32_t mbins, const CentPlan &plan,
                         int32_t device, double *entropy, double *ylim_out, int32_t *degenerate_out, int32_t *hist_out) {
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    Record rec; DevOut dent;
    DevBuf dscan, dvbin, dfreq, dlim, dhist;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, nullptr, N, ns, device, s));
    LPVS_TRY(dent.set(entropy, Nf * ns));
    // the tail of the small record: the keys of the extremes (2 ns); no moments: nothing is weighted or centred
    LPVS_TRY(rec.alloc_small((size_t)(2 * ns), false));
    unsigned long long *lim_dev = rec.tail<unsigned long long>();
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)(3 * ns * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    LPVS_TRY(rec.check("conditional_entropy", WeightSum::unused));
    LPVS_TRY(clock.mark(1));
    LPVS_TRY(dvbin.alloc((size_t)(N * ns)));
    LPVS_TRY(dlim.alloc(sizeof(double) * (size_t)(2 * ns) + sizeof(int32_t) * (size_t)ns));
    double *ylim_dev = dlim.as<double>();
    int32_t *deg_dev = reinterpret_cast<int32_t *>(ylim_dev + 2 * ns);
    LPVS_TRY(launch_cent_prepare(rec.y.p, N, ns, mbins, lim_dev, dvbin.as<unsigned char>(), ylim_dev, deg_dev, s));
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, f, sizeof(double) * (size_t)Nf, s));
    const int64_t nhist = Nf * ns * plan.cells;
    if (hist_out) LPVS_TRY(dhist.alloc(sizeof(int32_t) * (size_t)nhist));
    CentArgs A;
    A.t = rec.t.p; A.f = dfreq.as<double>(); A.vbin = dvbin.as<unsigned char>(); A.lim = lim_dev;
    A.N = N; A.Nf = Nf; A.ns = (int)ns; A.nbins = nbins; A.mbins = mbins;
    A.entropy = dent.p; A.hist = hist_out ? dhist.as<int32_t>() : nullptr;
    LPVS_TRY(clock.mark(2));
    LPVS_TRY(launch_cent(A, plan, s));
    LPVS_TRY(clock.mark(3));
    LPVS_TRY(copy_from_device(ylim_out, ylim_dev, sizeof(double) * (size_t)(2 * ns), s));
    LPVS_TRY(copy_from_device(degenerate_out, deg_dev, sizeof(int32_t) * (size_t)ns, s));
    if (hist_out) LPVS_TRY(copy_from_device(hist_out, dhist.p, sizeof(int32_t) * (size_t)nhist, s));
    LPVS_TRY(dent.finish(s));
    LPVS_TRY(clock.finish());
    int64_t ndeg = 0;
    for (int64_t c = 0; c < ns; ++c) ndeg += degenerate_out[c] != 0;
    double *g = g_cent_timing;
    g[0] = plan.F; g[1] = plan.ts; g[2] = plan.passes; g[3] = (double)plan.lds_bytes; g[4] = plan.copies; g[5] = g[6] = g[7] = 0;
    g[8] = (double)ndeg; g[9] = 1; g[15] = (double)Nf;
    for (int i = 0; i < 4; ++i) g[10 + i] = clock.ms(i);
    g[14] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_cent_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *f, int64_t Nf, int32_t nbins, int32_t mbins, int32_t device,
                      double *entropy_out, double *ylim_out, int32_t *degenerate_out, int32_t *hist_out) {
    try {
        if (!y || !t || !f || !entropy_out || !ylim_out || !degenerate_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (is_device_ptr(f) || is_device_ptr(ylim_out) || is_device_ptr(degenerate_out) || (hist_out && is_device_ptr(hist_out))) {
            set_error("conditional_entropy: f, ylim_out, degenerate_out and hist_out are host memory"); return LPVS_EARGUMENT;
        }
        const char *knob = experiment_env("LPVS_CENT_COPIES");
        const CentPlan plan = cent_plan(N, ns, f, Nf, nbins, mbins, knob ? atoll(knob) : 0);   // (the counts are checked before an array is read)
        if (plan.status != kFoldOk) { set_error("%s", plan.why.c_str()); return plan.status == kFoldArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        return cent_impl(y, ns, t, N, f, Nf, nbins, mbins, plan, device, entropy_out, ylim_out, degenerate_out, hist_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_cent_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_cent_timing, 16);
}

// ---- CLEAN (clean.hip; the decisions: clean_plan.h) ------------------------------------------------------------------------------------------
// what lpvs_clean_last_timing reports of the calling thread's last call of any of the four entries (0 where the call had no such stage):
// [0] path of the sums (1 direct, 2 transforms), [1] where the residual lived (1 LDS, 2 global memory), [2] threads of the loop's workgroup,
// [3] its LDS bytes, [4], [5] the fewest and the most iterations of a signal, [6] admissible bins, ms of [7] staging, the scan and the
// moments, [8] the sums, [9] the loop, [10] the restoration, [11] the copy-out, [12] total, [13] sigma of the beam
static thread_local double g_clean_timing[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

namespace {

typedef PhaseClock<6> CleanClock;   // marks: 0 start, 1 staged, 2 sums, 3 loop, 4 restoration, 5 (finish) copy-out

void clean_report(const CleanClock &clock, int taken, const CleanPlan *plan, int64_t itmin, int64_t itmax, int nadm, double sigma) {
    double *g = g_clean_timing;
    g[0] = taken; g[1] = plan ? plan->residual : 0; g[2] = plan ? plan->threads : 0; g[3] = plan ? (double)plan->lds_bytes : 0;
    g[4] = (double)itmin; g[5] = (double)itmax; g[6] = nadm;
    for (int i = 0; i < 5; ++i) g[7 + i] = clock.ms(i);
    g[12] = clock.total(); g[13] = sigma;
}
int32_t clean_refuse(int status, const std::string &why) {
    set_error("%s", why.c_str());
    return status == kCleanArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED;
}
// the grid of the dirty stage: f_m = m df (the double product), m = 0 .. 2 Nf - 2
std::vector<double> clean_grid(double df, int64_t Nf) {
    std::vector<double> hf((size_t)(2 * Nf - 1));
    for (size_t m = 0; m < hf.size(); ++m) hf[m] = (double)m * df;
    return hf;
}

// the record's front end, lomb.hip's sums on the grid and the repacking: Wn[2 Nf - 1], D[ns][Nf] (device); marks 1 before the sums
int32_t clean_dirty_stage(const char *who, Record &rec, LombSums &ls, DevBuf &dpart, const std::vector<double> &hf, int64_t Nf, bool center, int32_t path,
                          CleanClock &clock, double *Wn_dev, double *D_dev) {
    LPVS_TRY(rec.alloc_small(0));
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)(3 * rec.ns * lomb_sum_slabs(rec.N))));
    LPVS_TRY(rec.scan(dpart.as<double>()));
    LPVS_TRY(rec.check(who, WeightSum::positive));
    LPVS_TRY(rec.moments(center, dpart.as<double>()));
    LPVS_TRY(ls.choose(rec, hf, path));
    LPVS_TRY(clock.mark(1));
    LPVS_TRY(ls.run(rec, hf));
    return launch_clean_repack(ls.sums.as<double>(), Nf, rec.ns, Wn_dev, D_dev, rec.s);
}

struct CleanLoopInfo { int nadm = 0; int64_t itmin = 0, itmax = 0; };
// the loop on device spectra: R, C (device), pickval (device; nullptr with niter = 0); picks_out, iters_out, status_out: host
int32_t clean_loop_stage(const char *who, const double *D, const double *Wn, int64_t ns, int64_t Nf, double gain, int64_t niter, double tol, const CleanPlan &plan,
                         DevBuf &dwork, double *R, double *C, double *pickval, int32_t *picks_out, int32_t *iters_out, int32_t *status_out, hipStream_t s,
                         CleanLoopInfo *info) {
    // [den: Nf doubles | flags, admissible bins, iters[ns], status[ns], picks[ns niter]: ints | mask: Nf bytes]
    const size_t nints = (size_t)(2 + 2 * ns + ns * niter);
    LPVS_TRY(dwork.alloc(sizeof(double) * (size_t)Nf + sizeof(int32_t) * nints + (size_t)Nf));
    double *den = dwork.as<double>();
    int *flags_dev = reinterpret_cast<int *>(den + Nf), *nadm_dev = flags_dev + 1;
    int32_t *iters_dev = nadm_dev + 1, *status_dev = iters_dev + ns, *picks_dev = status_dev + ns;
    unsigned char *mask = reinterpret_cast<unsigned char *>(flags_dev + nints);
    LPVS_HIP(hipMemsetAsync(flags_dev, 0, sizeof(int), s));
    LPVS_TRY(launch_clean_finite(D, 2 * ns * Nf, flags_dev, s));
    LPVS_TRY(launch_clean_finite(Wn, 2 * (2 * Nf - 1), flags_dev, s));
    int flags = 0;
    LPVS_TRY(copy_from_device(&flags, flags_dev, sizeof(int), s));
    if (flags & 1) { set_error("%s: D or Wn holds a value that is not finite", who); return LPVS_EARGUMENT; }
    LPVS_TRY(launch_clean_prologue(Wn, Nf, den, mask, nadm_dev, s));
    LPVS_HIP(hipMemsetAsync(C, 0, sizeof(double) * (size_t)(2 * ns * Nf), s));
    if (niter > 0) {
        LPVS_HIP(hipMemsetAsync(picks_dev, 0xff, sizeof(int32_t) * (size_t)(ns * niter), s));             // -1: no pick
        LPVS_HIP(hipMemsetAsync(pickval, 0, sizeof(double) * (size_t)(2 * ns * niter), s));
    }
    LPVS_TRY(launch_clean_loop(D, Wn, den, mask, ns, Nf, gain, niter, tol, plan, R, C, picks_dev, pickval, iters_dev, status_dev, s));
    LPVS_TRY(copy_from_device(&info->nadm, nadm_dev, sizeof(int), s));
    LPVS_TRY(copy_from_device(iters_out, iters_dev, sizeof(int32_t) * (size_t)ns, s));
    LPVS_TRY(copy_from_device(status_out, status_dev, sizeof(int32_t) * (size_t)ns, s));
    if (niter > 0) LPVS_TRY(copy_from_device(picks_out, picks_dev, sizeof(int32_t) * (size_t)(ns * niter), s));
    info->itmin = info->itmax = iters_out[0];
    for (int64_t c = 1; c < ns; ++c) {
        if (iters_out[c] < info->itmin) info->itmin = iters_out[c];
        if (iters_out[c] > info->itmax) info->itmax = iters_out[c];
    }
    return LPVS_OK;
}

// S[ns][Nf] (device) from R, C (device)
int32_t clean_restore_stage(const double *R, const double *C, int64_t ns, int64_t Nf, double df, double sigma, DevBuf &dwork, double *S, hipStream_t s) {
    // [beam: 2 Nf - 1 doubles | list: ns Nf ints | count: ns ints]
    const int64_t M = 2 * Nf - 1;
    LPVS_TRY(dwork.alloc(sizeof(double) * (size_t)M + sizeof(int32_t) * (size_t)(ns * Nf + ns)));
    double *beam = dwork.as<double>();
    int32_t *list = reinterpret_cast<int32_t *>(beam + M), *count = list + ns * Nf;
    return launch_clean_restore(R, C, ns, Nf, df, sigma, list, count, beam, S, s);
}

bool clean_force_global() {
    const char *knob = experiment_env("LPVS_CLEAN_RESIDUAL");
    return knob && !strcmp(knob, "global");
}
int32_t clean_check_record(const char *who, int64_t N, int32_t path) {
    if (N <= 0) { set_error("%s: need N > 0 (N = %lld)", who, (long long)N); return LPVS_EARGUMENT; }
    if (path < kLombPathAuto || path > kLombPathNufft) { set_error("path must be 0 (auto), 1 (direct) or 2 (NUFFT), got %d", path); return LPVS_EARGUMENT; }
    return LPVS_OK;
}

}  // namespace

int32_t lpvs_dirty_spectrum_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, double df, int64_t Nf, int32_t center_data, int32_t path,
                                int32_t device, double *D_out, double *Wn_out) {
    try {
        if (!y || !t || !D_out || !Wn_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        int status = kCleanOk; std::string why;
        if (!clean_check_sizes("dirty_spectrum", ns, Nf, &status, &why) || !clean_check_df("dirty_spectrum", df, &status, &why)) return clean_refuse(status, why);
        LPVS_TRY(clean_check_record("dirty_spectrum", N, path));
        const std::vector<double> hf = clean_grid(df, Nf);
        LPVS_TRY(Record::admit(device));
        hipStream_t s = nullptr;
        CleanClock clock;
        LPVS_TRY(clock.init(s));
        Record rec; DevOut dD, dWn;
        DevBuf dpart; LombSums ls;
        DrainOnExit drain(s);
        LPVS_TRY(clock.mark(0));
        LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
        LPVS_TRY(dD.set(D_out, 2 * ns * Nf));
        LPVS_TRY(dWn.set(Wn_out, 2 * (2 * Nf - 1)));
        LPVS_TRY(clean_dirty_stage("dirty_spectrum", rec, ls, dpart, hf, Nf, center_data != 0, path, clock, dWn.p, dD.p));
        for (int i = 2; i <= 4; ++i) LPVS_TRY(clock.mark(i));
        LPVS_TRY(dD.finish(s));
        LPVS_TRY(dWn.finish(s));
        LPVS_TRY(clock.finish());
        clean_report(clock, ls.taken, nullptr, 0, 0, 0, 0.0);
        return LPVS_OK;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_clean_loop_f64(const double *D, int64_t ns, int64_t Nf, const double *Wn, double gain, int64_t niter, double tol, int32_t device, double *R_out,
                            double *C_out, int32_t *picks_out, double *pickval_out, int32_t *iters_out, int32_t *status_out) {
    try {
        if (!D || !Wn || !R_out || !C_out || !picks_out || !pickval_out || !iters_out || !status_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        if (is_device_ptr(picks_out) || is_device_ptr(iters_out) || is_device_ptr(status_out)) {
            set_error("clean: picks_out, iters_out and status_out are host memory"); return LPVS_EARGUMENT;
        }
        const CleanPlan plan = clean_plan(ns, Nf, gain, niter, tol, clean_force_global());
        if (plan.status != kCleanOk) return clean_refuse(plan.status, plan.why);
        LPVS_TRY(Record::admit(device));
        hipStream_t s = nullptr;
        CleanClock clock;
        LPVS_TRY(clock.init(s));
        Staged<double> sD, sWn; DevOut dR, dC, dpv;
        DevBuf dwork;
        DrainOnExit drain(s);
        LPVS_TRY(clock.mark(0));
        LPVS_TRY(sD.set(D, 2 * ns * Nf, device, s));
        LPVS_TRY(sWn.set(Wn, 2 * (2 * Nf - 1), device, s));
        LPVS_TRY(dR.set(R_out, 2 * ns * Nf));
        LPVS_TRY(dC.set(C_out, 2 * ns * Nf));
        if (niter > 0) LPVS_TRY(dpv.set(pickval_out, 2 * ns * niter));
        LPVS_TRY(clock.mark(1));
        LPVS_TRY(clock.mark(2));
        CleanLoopInfo info;
        LPVS_TRY(clean_loop_stage("clean", sD.p, sWn.p, ns, Nf, gain, niter, tol, plan, dwork, dR.p, dC.p, dpv.p, picks_out, iters_out, status_out, s, &info));
        LPVS_TRY(clock.mark(3));
        LPVS_TRY(clock.mark(4));
        LPVS_TRY(dR.finish(s));
        LPVS_TRY(dC.finish(s));
        if (niter > 0) LPVS_TRY(dpv.finish(s));
        LPVS_TRY(clock.finish());
        clean_report(clock, 0, &plan, info.itmin, info.itmax, info.nadm, 0.0);
        return LPVS_OK;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_clean_restore_f64(const double *R, const double *C, int64_t ns, int64_t Nf, double df, double sigma, int32_t device, double *S_out) {
    try {
        if (!R || !C || !S_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        int status = kCleanOk; std::string why;
        if (!clean_check_sizes("clean_restore", ns, Nf, &status, &why) || !clean_check_df("clean_restore", df, &status, &why)) return clean_refuse(status, why);
        if (!(sigma > 0.0) || !std::isfinite(sigma)) { set_error("clean_restore: sigma must be positive and finite, got %g", sigma); return LPVS_EARGUMENT; }
        LPVS_TRY(Record::admit(device));
        hipStream_t s = nullptr;
        CleanClock clock;
        LPVS_TRY(clock.init(s));
        Staged<double> sR, sC; DevOut dS;
        DevBuf dwork;
        DrainOnExit drain(s);
        LPVS_TRY(clock.mark(0));
        LPVS_TRY(sR.set(R, 2 * ns * Nf, device, s));
        LPVS_TRY(sC.set(C, 2 * ns * Nf, device, s));
        LPVS_TRY(dS.set(S_out, 2 * ns * Nf));
        for (int i = 1; i <= 3; ++i) LPVS_TRY(clock.mark(i));
        LPVS_TRY(clean_restore_stage(sR.p, sC.p, ns, Nf, df, sigma, dwork, dS.p, s));
        LPVS_TRY(clock.mark(4));
        LPVS_TRY(dS.finish(s));
        LPVS_TRY(clock.finish());
        clean_report(clock, 0, nullptr, 0, 0, 0, sigma);
        return LPVS_OK;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_clean_f64(const double *y, int64_t ns, const double *t, int64_t N, const double *W, double df, int64_t Nf, int32_t center_data, int32_t path, double gain,
                       int64_t niter, double tol, double sigma, int32_t device, double *D_out, double *Wn_out, double *R_out, double *C_out, int32_t *picks_out,
                       double *pickval_out, int32_t *iters_out, int32_t *status_out, double *S_out, double *sigma_out) {
    try {
        if (!y || !t || !D_out || !Wn_out || !R_out || !C_out || !picks_out || !pickval_out || !iters_out || !status_out || !S_out) {
            set_error("NULL argument"); return LPVS_EARGUMENT;
        }
        if (is_device_ptr(picks_out) || is_device_ptr(iters_out) || is_device_ptr(status_out) || (sigma_out && is_device_ptr(sigma_out))) {
            set_error("clean: picks_out, iters_out, status_out and sigma_out are host memory"); return LPVS_EARGUMENT;
        }
        const CleanPlan plan = clean_plan(ns, Nf, gain, niter, tol, clean_force_global());
        if (plan.status != kCleanOk) return clean_refuse(plan.status, plan.why);
        int status = kCleanOk; std::string why;
        if (!clean_check_df("clean", df, &status, &why)) return clean_refuse(status, why);
        if (!(sigma >= 0.0) || !std::isfinite(sigma)) { set_error("clean: sigma must be finite and positive, or 0 to fit it, got %g", sigma); return LPVS_EARGUMENT; }
        LPVS_TRY(clean_check_record("clean", N, path));
        const std::vector<double> hf = clean_grid(df, Nf);
        LPVS_TRY(Record::admit(device));
        hipStream_t s = nullptr;
        CleanClock clock;
        LPVS_TRY(clock.init(s));
        Record rec; DevOut dD, dWn, dR, dC, dpv, dS;
        DevBuf dpart, dloop, drest; LombSums ls;
        DrainOnExit drain(s);
        LPVS_TRY(clock.mark(0));
        LPVS_TRY(rec.stage(t, y, W, N, ns, device, s));
        LPVS_TRY(dD.set(D_out, 2 * ns * Nf));
        LPVS_TRY(dWn.set(Wn_out, 2 * (2 * Nf - 1)));
        LPVS_TRY(dR.set(R_out, 2 * ns * Nf));
        LPVS_TRY(dC.set(C_out, 2 * ns * Nf));
        if (niter > 0) LPVS_TRY(dpv.set(pickval_out, 2 * ns * niter));
        LPVS_TRY(dS.set(S_out, 2 * ns * Nf));
        LPVS_TRY(clean_dirty_stage("clean", rec, ls, dpart, hf, Nf, center_data != 0, path, clock, dWn.p, dD.p));
        LPVS_TRY(clock.mark(2));
        CleanLoopInfo info;
        LPVS_TRY(clean_loop_stage("clean", dD.p, dWn.p, ns, Nf, gain, niter, tol, plan, dloop, dR.p, dC.p, dpv.p, picks_out, iters_out, status_out, s, &info));
        LPVS_TRY(clock.mark(3));
        if (sigma == 0.0) {                                                   // the beam's width from the window (clean_plan.h: clean_sigma)
            std::vector<double> hWn((size_t)(2 * (2 * Nf - 1)));
            LPVS_TRY(copy_from_device(hWn.data(), dWn.p, sizeof(double) * hWn.size(), s));
            sigma = clean_sigma(hWn.data(), Nf, df);
            if (!(sigma > 0.0) || !std::isfinite(sigma)) { set_error("clean: the fitted sigma of the beam is %g", sigma); return LPVS_ENUMERIC; }
        }
        if (sigma_out) *sigma_out = sigma;
        LPVS_TRY(clean_restore_stage(dR.p, dC.p, ns, Nf, df, sigma, drest, dS.p, s));
        LPVS_TRY(clock.mark(4));
        LPVS_TRY(dD.finish(s));
        LPVS_TRY(dWn.finish(s));
        LPVS_TRY(dR.finish(s));
        LPVS_TRY(dC.finish(s));
        if (niter > 0) LPVS_TRY(dpv.finish(s));
        LPVS_TRY(dS.finish(s));
        LPVS_TRY(clock.finish());
        clean_report(clock, ls.taken, &plan, info.itmin, info.itmax, info.nadm, sigma);
        return LPVS_OK;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_clean_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_clean_timing, 14);
}

// ---- the bootstrap of the Lomb-Scargle periodogram (lomb_boot.hip; the decisions: lomb_boot_plan.h) ------------------------------------------
// what lpvs_lombscargle_bootstrap_last_timing reports of the calling thread's last call: [0] resamples, [1] chunks, [2] resamples per thread
// (TS), [3] slab length, [4] slabs, [5] degenerate frequencies, ms of [6] staging, the scan and the shared sums of the record, [7] the
// moments of the resamples, [8] the bootstrap sums, [9] the epilogue and the maxima, [10] the copy-out, [11] total
static thread_local double g_lomb_boot_timing[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static int32_t lomb_boot_impl(const double *y, const double *t, int64_t N, const double *W, const std::vector<double> &hf, int64_t B, int64_t seed, int64_t row0,
                              bool fit_mean, bool center, bool psd, int32_t device, const LombBootPlan &plan, double *max_out, int64_t *argmax_out, double *mean_out,
                              double *power_out) {
    const int64_t Nf = (int64_t)hf.size();
    LPVS_TRY(Record::admit(device));
    hipStream_t s = nullptr;
    PhaseClock<5> clock;
    LPVS_TRY(clock.init(s));
    struct ChunkEvents {                                                     // a chunk: before its sums, between sums and epilogue, after the epilogue
        hipEvent_t a = nullptr, b = nullptr, c = nullptr;
        ~ChunkEvents() { for (hipEvent_t x : {a, b, c}) if (x) (void)hipEventDestroy(x); }
    };
    std::vector<ChunkEvents> cev((size_t)plan.nchunks);
    Record rec; DevOut dmax, dpower;
    DevBuf dscan, dshared, dfreq, dslab, dmom, dargmax, dpart, dsums;
    DrainOnExit drain(s);
    LPVS_TRY(clock.mark(0));
    LPVS_TRY(rec.stage(t, y, W, N, 1, device, s));
    LPVS_TRY(dmax.set(max_out, B));
    if (power_out) LPVS_TRY(dpower.set(power_out, Nf * B));
    // the observed record, as g4 takes it: the scan (sum W, the refusals), the normalised weights, and C, S, C2, S2 by the direct path's
    // kernels with one signal (no tail of the small record; the degenerate count is the spare int of its flags word)
    LPVS_TRY(rec.alloc_small(0));
    int *ndeg_dev = rec.flags_dev + 1;
    LPVS_TRY(dscan.alloc(sizeof(double) * (size_t)(3 * lomb_sum_slabs(N))));
    LPVS_TRY(rec.scan(dscan.as<double>()));
    LPVS_TRY(rec.check("lombscargle", WeightSum::positive));
    LPVS_TRY(rec.moments(center, dscan.as<double>()));
    const LombTiling tl = lomb_tiling(N, Nf, 1);
    LPVS_TRY(dfreq.alloc(sizeof(double) * (size_t)Nf));
    LPVS_TRY(copy_to_device(dfreq.p, hf.data(), sizeof(double) * (size_t)Nf, s));
    LPVS_TRY(dslab.alloc(sizeof(double) * (size_t)(tl.nslab * 6 * Nf)));
    LPVS_TRY(dshared.alloc(sizeof(double) * (size_t)(6 * Nf)));              // rows C, S, C2, S2 (and the record's own YC, YS, not used)
    LPVS_TRY(launch_lomb_direct(rec.t.p, rec.w.as<double>(), rec.wy.as<double>(), N, 1, dfreq.as<double>(), Nf, tl, dslab.as<double>(), dshared.as<double>(), s));
    dslab.release();
    LPVS_TRY(clock.mark(1));
    // the resamples' moments: mean[B], then {Y, YY, R, -} per resample
    LPVS_TRY(dmom.alloc(sizeof(double) * (size_t)(5 * B)));
    double *mean_dev = dmom.as<double>(), *mom_dev = mean_dev + B;
    LPVS_TRY(dargmax.alloc(sizeof(int64_t) * (size_t)B));
    LPVS_TRY(launch_lomb_boot_moments(rec.y.p, rec.w.as<double>(), N, seed, row0, B, center, mean_dev, mom_dev, s));
    LPVS_TRY(clock.mark(2));
    LPVS_HIP(hipMemsetAsync(ndeg_dev, 0, sizeof(int), s));
    LPVS_TRY(dpart.alloc(sizeof(double) * (size_t)plan.part_doubles));
    LPVS_TRY(dsums.alloc(sizeof(double) * (size_t)(2 * plan.chunk * Nf)));
    for (int64_t c = 0; c < plan.nchunks; ++c) {
        const int64_t r0 = c * plan.chunk, count = c + 1 < plan.nchunks ? plan.chunk : plan.last_chunk;
        ChunkEvents &ce = cev[(size_t)c];
        LPVS_HIP(hipEventCreate(&ce.a)); LPVS_HIP(hipEventCreate(&ce.b)); LPVS_HIP(hipEventCreate(&ce.c));
        LPVS_HIP(hipEventRecord(ce.a, s));
        LPVS_TRY(launch_lomb_boot_sums(rec.t.p, rec.w.as<double>(), rec.y.p, N, seed, row0, r0, count, center ? mean_dev : nullptr, dfreq.as<double>(), Nf, plan,
                                       dpart.as<double>(), dsums.as<double>(), s));
        LPVS_HIP(hipEventRecord(ce.b, s));
        LPVS_TRY(launch_lomb_boot_epilogue(dshared.as<double>(), dsums.as<double>(), Nf, r0, count, mean_dev, mom_dev, fit_mean, center, psd, N,
                                           power_out ? dpower.p : nullptr, dmax.p, dargmax.as<int64_t>(), c == 0, ndeg_dev, s));
        LPVS_HIP(hipEventRecord(ce.c, s));
    }
    LPVS_TRY(clock.mark(3));
    int ndeg = 0;
    LPVS_TRY(copy_from_device(&ndeg, ndeg_dev, sizeof(int), s));
    if (argmax_out) LPVS_TRY(copy_from_device(argmax_out, dargmax.p, sizeof(int64_t) * (size_t)B, s));
    if (mean_out) LPVS_TRY(copy_from_device(mean_out, mean_dev, sizeof(double) * (size_t)B, s));
    LPVS_TRY(dmax.finish(s));
    if (power_out) LPVS_TRY(dpower.finish(s));
    LPVS_TRY(clock.finish());
    double sums_ms = 0, epi_ms = 0;
    for (int64_t c = 0; c < plan.nchunks; ++c) {
        float x = 0, z = 0;
        LPVS_HIP(hipEventElapsedTime(&x, cev[(size_t)c].a, cev[(size_t)c].b));
        LPVS_HIP(hipEventElapsedTime(&z, cev[(size_t)c].b, cev[(size_t)c].c));
        sums_ms += x; epi_ms += z;
    }
    double *g = g_lomb_boot_timing;
    g[0] = (double)B; g[1] = (double)plan.nchunks; g[2] = plan.ts; g[3] = (double)plan.slab_samples; g[4] = (double)plan.nslab; g[5] = ndeg;
    g[6] = clock.ms(0); g[7] = clock.ms(1); g[8] = sums_ms; g[9] = epi_ms; g[10] = clock.ms(3); g[11] = clock.total();
    return LPVS_OK;
}

int32_t lpvs_lombscargle_bootstrap_f64(const double *y, const double *t, int64_t N, const double *W, const double *f, int64_t Nf, int64_t B, int64_t seed, int64_t row0,
                                       int32_t fit_mean, int32_t center_data, int32_t normalization, int32_t device, double *max_out, int64_t *argmax_out,
                                       double *mean_out, double *power_out) {
    try {
        if (!y || !t || !f || !max_out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
        const char *ts_knob = experiment_env("LPVS_LOMB_BOOT_TS"), *mb_knob = experiment_env("LPVS_LOMB_BOOT_MB");
        const LombBootPlan plan = lomb_boot_plan(N, Nf, B, row0, ts_knob ? atoll(ts_knob) : 0, mb_knob ? atof(mb_knob) : 0.0);
        if (plan.status != kLombBootOk) { set_error("%s", plan.why.c_str()); return plan.status == kLombBootArgument ? LPVS_EARGUMENT : LPVS_EUNSUPPORTED; }
        LPVS_TRY(check_normalization(normalization));
        if (is_device_ptr(f) || (argmax_out && is_device_ptr(argmax_out)) || (mean_out && is_device_ptr(mean_out))) {
            set_error("lombscargle_bootstrap: f, argmax_out and mean_out are host memory"); return LPVS_EARGUMENT;
        }
        std::vector<double> hf;
        LPVS_TRY(host_frequencies(f, Nf, hf));
        return lomb_boot_impl(y, t, N, W, hf, B, seed, row0, fit_mean != 0, center_data != 0, normalization == LPVS_LOMB_PSD, device, plan, max_out, argmax_out,
                              mean_out, power_out);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}

int32_t lpvs_lombscargle_bootstrap_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_lomb_boot_timing, 12);
}
