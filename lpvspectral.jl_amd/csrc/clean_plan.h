// clean_plan.h -- the host-side decisions of CLEAN (clean.hip, uneven.hip; include/lpvspectral.h g11): the checks of the
// host arguments with their messages, the threads of the loop's workgroup, where the residual lives and the LDS bytes.  Pure functions of
// numbers: uneven.hip and clean.hip allocate and launch what they say and decide none of this themselves.
// No HIP dependency: the host-side test (tests/test_clean_plan.py) compiles it as it is.
//
// THE LOOP is one workgroup per signal and one launch for all its iterations (clean.hip).  Bin k of the residual belongs to thread
// k mod threads for the whole launch, so no thread ever reads a residual another one wrote: the peak's value travels with the arg-max.
//   threads   ceil(Nf / 4) rounded up to whole waves of 64, at least 64 and at most 1024: about four bins per thread.  The loop is bound
//             by the latency of one pass, not by throughput; more threads shorten the pass until the arg-max over the waves costs more
//             than it saves.
//   residual  in LDS where its 16 Nf bytes are at most kCleanLdsBudget = 128 KiB of the CU's 160 KiB (Nf <= 8192), in global memory (the
//             R_out block itself) otherwise, or when the experiment knob LPVS_CLEAN_RESIDUAL=global says so.  The results are the same
//             bits: it is the same code through a pointer.
//   lds_bytes the residual, if it is there, and kCleanSlotBytes = 2 x 16 x 32 for the arg-max: one {P, Re R, Im R, k} per wave, twice,
//             so that an iteration needs ONE barrier (iteration i writes the set i mod 2 while set (i - 1) mod 2 may still be read).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

namespace lpvs {

enum { kCleanOk = 0, kCleanArgument = 1, kCleanUnsupported = 2 };
enum { kCleanStatusNiter = 0, kCleanStatusTol = 1, kCleanStatusEmpty = 2 };     // why a signal's loop ended (status_out)
enum { kCleanResidualLds = 1, kCleanResidualGlobal = 2 };

constexpr int64_t kCleanMaxFreqs = (int64_t)1 << 20, kCleanMaxIters = (int64_t)1 << 24, kCleanMaxPicks = (int64_t)1 << 28;
constexpr int64_t kCleanLdsBudget = 128 * 1024;
constexpr int kCleanMaxThreads = 1024, kCleanBinsPerThread = 4, kCleanSlotBytes = 2 * 16 * 32;
// a bin p is admissible iff den_p = 1 - |Wn_2p|^2 >= 2^-20
constexpr double kCleanMinDen = 1.0 / 1048576.0;

struct CleanPlan {
    int status = kCleanArgument;
    std::string why;                    // (refused: the reason)
    int threads = 0, residual = 0;
    int64_t lds_bytes = 0, workgroups = 0;
};

// the checks of the sizes alone (lpvs_dirty_spectrum_f64 and lpvs_clean_restore_f64 have no loop); who: the entry's name
inline bool clean_check_sizes(const char *who_, int64_t ns, int64_t Nf, int *status, std::string *why) {
    const std::string who(who_);
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (ns < 1 || ns > 65535) { *status = kCleanArgument; *why = who + ": need 1 <= ns <= 65535 (ns = " + ll(ns) + ")"; return false; }
    if (Nf < 2) { *status = kCleanArgument; *why = who + ": Nf must be at least 2, got " + ll(Nf); return false; }
    if (Nf > kCleanMaxFreqs) { *status = kCleanUnsupported; *why = who + ": " + ll(Nf) + " frequencies are more than 2^20"; return false; }
    return true;
}
inline bool clean_check_df(const char *who_, double df, int *status, std::string *why) {
    if (!(df > 0.0) || !std::isfinite(df)) {
        *status = kCleanArgument;
        *why = std::string(who_) + ": df must be positive and finite, got " + std::to_string(df);
        return false;
    }
    return true;
}

// force_global: LPVS_CLEAN_RESIDUAL=global
inline CleanPlan clean_plan(int64_t ns, int64_t Nf, double gain, int64_t niter, double tol, bool force_global) {
    CleanPlan p;
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (!clean_check_sizes("clean", ns, Nf, &p.status, &p.why)) return p;
    if (niter < 0) { p.status = kCleanArgument; p.why = "clean: niter must not be negative, got " + ll(niter); return p; }
    if (niter > kCleanMaxIters) { p.status = kCleanUnsupported; p.why = "clean: " + ll(niter) + " iterations are more than 2^24"; return p; }
    if (!(gain > 0.0 && gain < 2.0)) { p.status = kCleanArgument; p.why = "clean: gain must lie in (0, 2), got " + std::to_string(gain); return p; }
    if (!(tol >= 0.0 && tol < 1.0)) { p.status = kCleanArgument; p.why = "clean: tol must lie in [0, 1), got " + std::to_string(tol); return p; }
    if (ns * niter > kCleanMaxPicks) {
        p.status = kCleanUnsupported;
        p.why = "clean: " + ll(ns) + " signals times " + ll(niter) + " iterations are more than 2^28 picks";
        return p;
    }
    int64_t t = (Nf + kCleanBinsPerThread - 1) / kCleanBinsPerThread;
    t = (t + 63) / 64 * 64;
    p.threads = (int)(t < 64 ? 64 : t > kCleanMaxThreads ? kCleanMaxThreads : t);
    p.residual = !force_global && 16 * Nf <= kCleanLdsBudget ? kCleanResidualLds : kCleanResidualGlobal;
    p.lds_bytes = kCleanSlotBytes + (p.residual == kCleanResidualLds ? 16 * Nf : 0);
    p.workgroups = ns;
    p.status = kCleanOk;
    return p;
}

// The width of the restoring beam from the spectral window: the first m >= 1 with P_m = Re Wn_m^2 + Im Wn_m^2 < 1/2 (the half-power point
// of the main lobe), interpolated linearly in P between m - 1 and m, is the half width h = ((m - 1) + (P_{m-1} - 1/2) / (P_{m-1} - P_m)) df;
// sigma = h / sqrt(2 ln 2), the Gaussian with that half width at half maximum.  No such m (a window that never falls): h = 2 (Nf - 1) df.
// Wn: 2 Nf - 1 interleaved complex values.  Every operation is a rounded double operation in the order written (the Python layer does the same).
constexpr double kCleanHwhmToSigma = 0.8493218002880191;                      // 1 / sqrt(2 ln 2)
inline double clean_sigma(const double *Wn, int64_t Nf, double df) {
    const int64_t M = 2 * Nf - 1;
    double prev = Wn[0] * Wn[0] + Wn[1] * Wn[1];
    for (int64_t m = 1; m < M; ++m) {
        const double P = Wn[2 * m] * Wn[2 * m] + Wn[2 * m + 1] * Wn[2 * m + 1];
        if (P < 0.5) {
            const double frac = prev > P ? (prev - 0.5) / (prev - P) : 0.0;
            const double h = ((double)(m - 1) + frac) * df;
            return h * kCleanHwhmToSigma;
        }
        prev = P;
    }
    return ((double)(M - 1) * df) * kCleanHwhmToSigma;
}

}  // namespace lpvs
