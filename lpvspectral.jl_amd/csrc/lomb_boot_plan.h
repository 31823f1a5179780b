// lomb_boot_plan.h -- the host-side decisions of the Lomb-Scargle bootstrap (lombscargle_bootstrap: lomb_boot.hip, api.hip):
// how many resamples a thread of the bootstrap kernel carries, how the record is cut into slabs of samples, how the B resamples are cut
// into chunks whose partial sums stay under a budget, the grids, and what is refused.
// Pure functions of numbers: api.hip and lomb_boot.hip allocate and launch what they say and decide none of this themselves.
// No HIP dependency: the host-side test (tests/test_lomb_boot_plan.py) compiles it as it is.
#pragma once

#include <string>

#include "lomb_plan.h"

namespace lpvs {

// ---- resamples per thread ------------------------------------------------------------------------------------------------------------------
// A thread of the bootstrap kernel owns one frequency and one sample lane (as in lomb_direct_kernel) and carries the YC, YS accumulators
// of TS resamples: one sincospi per (sample, frequency) serves TS resamples, 2 TS fused multiply-adds each.  Two instantiations, 8 and
// 16 (120 and 214 VGPRs, no scratch); 16 is the default: measured (profiles/lomb_boot_time.txt) it is ahead of 8 by up to 1.4 times
// wherever the sums dominate the call and level with it on the smallest shape.  LPVS_LOMB_BOOT_TS=8 (experiment knob) picks the other.
// Tried and dropped: TS = 32 and 8 resamples x 2 frequencies per thread, both slower than 16.
constexpr int kLombBootTs = 16;
inline int lomb_boot_ts(long long knob) { return knob == 8 || knob == 16 ? (int)knob : kLombBootTs; }

// ---- the slab of samples -------------------------------------------------------------------------------------------------------------------
// A function of N ALONE (never of B, Nf or the chunk): kLombBootSlab samples, longer only where the record would otherwise leave more
// than kLombMaxSlabs slabs (N > 2^20).  The order of every addition behind a resample's sums is that of its slabs, so it depends on N only.
constexpr int64_t kLombBootSlab = 1024;
static_assert(kLombBootSlab % kLombStage == 0, "the slab is staged kLombStage samples at a time");
inline int64_t lomb_boot_slab(int64_t N) {
    const int64_t s = round_up(ceil_div(N, kLombMaxSlabs), (int64_t)kLombStage);
    return s < kLombBootSlab ? kLombBootSlab : s;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------
// The partial sums of a chunk are nslab x 2 chunk x Nf doubles (YC, YS per resample, slab and frequency); the chunk is the largest
// multiple of TS that keeps them under the budget -- kLombBootBudgetMB, or LPVS_LOMB_BOOT_MB (experiment knob; fractions are allowed, so
// that tests cut small calls into several chunks) -- and at least one block of TS resamples whatever the budget says.
// The bootstrap kernel's grid is (tiles of frequencies x blocks of TS resamples, slabs); the moments and the epilogue take one
// workgroup per resample.
constexpr double kLombBootBudgetMB = 256.0;
constexpr int64_t kLombBootMaxSamples = (int64_t)1 << 31, kLombBootMaxFreqs = (int64_t)1 << 24, kLombBootMaxRow = (int64_t)1 << 40;
enum { kLombBootOk = 0, kLombBootArgument = 1, kLombBootUnsupported = 2 };
struct LombBootPlan {
    int status = kLombBootOk;
    std::string why;                    // (refused: the reason)
    int ts = 0;                         // resamples per thread
    int64_t slab_samples = 0, nslab = 0, ftiles = 0;
    int64_t chunk = 0, nchunks = 0, last_chunk = 0;   // resamples per chunk (a multiple of ts), chunks, resamples of the last one
    int64_t part_doubles = 0;           // nslab * 2 chunk * Nf
};
inline LombBootPlan lomb_boot_plan(int64_t N, int64_t Nf, int64_t B, int64_t row0, long long ts_knob, double budget_mb) {
    LombBootPlan p;
    auto refuse = [&p](int status, const std::string &why) { p.status = status; p.why = why; return p; };
    if (N < 1 || Nf < 1 || B < 1 || row0 < 0)
        return refuse(kLombBootArgument, "lombscargle_bootstrap: need N > 0, Nf > 0, B > 0 and row0 >= 0 (N = " + std::to_string(N) + ", Nf = " +
                                             std::to_string(Nf) + ", B = " + std::to_string(B) + ", row0 = " + std::to_string(row0) + ")");
    if (N >= kLombBootMaxSamples) return refuse(kLombBootUnsupported, "lombscargle_bootstrap: " + std::to_string(N) + " samples are 2^31 or more");
    if (Nf > kLombBootMaxFreqs) return refuse(kLombBootUnsupported, std::to_string(Nf) + " frequencies are too many");
    if (B > kLombBootMaxRow || row0 > kLombBootMaxRow - B)
        return refuse(kLombBootUnsupported, "lombscargle_bootstrap: the resamples " + std::to_string(row0) + " .. " + std::to_string(row0) + " + " +
                                                std::to_string(B) + " - 1 reach beyond 2^40");
    if (B > kLombMaxGrid)
        return refuse(kLombBootUnsupported, "lombscargle_bootstrap: " + std::to_string(B) + " resamples are more than one call takes (a workgroup each: at most " +
                                                std::to_string(kLombMaxGrid) + ")");
    p.ts = lomb_boot_ts(ts_knob);
    p.slab_samples = lomb_boot_slab(N);
    p.nslab = ceil_div(N, p.slab_samples);
    p.ftiles = ceil_div(Nf, kLombFreqTile);
    const double budget = (budget_mb > 0.0 ? budget_mb : kLombBootBudgetMB) * 1048576.0;
    const double per_resample = 8.0 * 2.0 * (double)p.nslab * (double)Nf;          // bytes of partial sums
    double fit = budget / per_resample;
    const double most = (double)round_up(B, (int64_t)p.ts);
    if (fit > most) fit = most;
    int64_t chunk = (int64_t)fit / p.ts * p.ts;
    if (chunk < p.ts) chunk = p.ts;                                                  // one block of TS resamples whatever the budget says
    const int64_t grid_most = kLombMaxGrid / p.ftiles * p.ts;                        // (tiles x blocks) in one grid dimension
    if (chunk > grid_most) chunk = grid_most;
    p.chunk = chunk;
    p.nchunks = ceil_div(B, chunk);
    p.last_chunk = B - (p.nchunks - 1) * chunk;
    p.part_doubles = p.nslab * 2 * chunk * Nf;
    return p;
}

}  // namespace lpvs
