// lomb_terms_plan.h -- the host-side decisions of the multi-harmonic Lomb-Scargle periodogram (lombscargle(..., nterms = K): lomb_terms.hip,
// api.hip; include/lpvspectral.h g7): how many signals a thread of the sums kernel carries, how many accumulators that
// makes, how frequencies and samples are tiled, how many rows of partial sums a slab leaves, the grids, and what is refused.
// Pure functions of numbers: api.hip and lomb_terms.hip allocate and launch what they say and decide none of this themselves.
// No HIP dependency: the host-side test (tests/test_lomb_terms_plan.py) compiles it as it is.
#pragma once

#include <string>

#include "lomb_plan.h"

namespace lpvs {

// ---- signals per thread --------------------------------------------------------------------------------------------------------------------
// A thread of lomb_terms_kernel<K, TS> owns one frequency and one sample lane (as in lomb_direct_kernel) and carries C_m, S_m of the
// harmonics m = 1 .. 2K (4K accumulators) and YC_h, YS_h, h = 1 .. K, of TS signals (2K TS): one sincospi and 2K - 1 complex rotations
// per (sample, frequency) serve them all.  TS is the largest of {4, 2, 1} that keeps the accumulators within kLombTermsMaxAcc doubles
// (96 of the thread's VGPRs), and 1 for a single signal.
constexpr int kLombMaxTerms = 6, kLombTermsMaxAcc = 48;
inline int lomb_terms_acc(int K, int ts) { return 4 * K + 2 * K * ts; }
inline int lomb_terms_ts(int K, int64_t ns) {
    if (ns <= 1) return 1;
    for (int ts = 4; ts > 1; ts /= 2)
        if (lomb_terms_acc(K, ts) <= kLombTermsMaxAcc) return ts;
    return 1;
}
// rows of sums per frequency: C_m, S_m (m = 1 .. 2K), then YC_h, YS_h (h = 1 .. K) of every signal
inline int64_t lomb_terms_rows(int K, int64_t ns) { return 4 * (int64_t)K + 2 * (int64_t)K * ns; }

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------
// Tiles of kLombFreqTile frequencies and slabs of samples come from lomb_tiling's rule: the slab is a function of N and Nf alone, so the
// order of every addition behind a column does not depend on which signals ride along (nor on K).  The sums kernel's grid is
// (tiles, slabs, blocks of TS signals); the slab sum takes a thread per element of rows x Nf, the epilogue a thread per (frequency, signal).
constexpr int64_t kLombTermsMaxFreqs = (int64_t)1 << 24, kLombTermsMaxSignals = 65535;
constexpr int kLombTermsEpilogueBlock = 64;
enum { kLombTermsOk = 0, kLombTermsArgument = 1, kLombTermsUnsupported = 2 };
struct LombTermsPlan {
    int status = kLombTermsOk;
    std::string why;                    // (refused: the reason)
    int K = 0, ts = 0, acc = 0, sblocks = 0;
    int64_t ftiles = 0, slab_samples = 0, nslab = 0;
    int64_t rows = 0;                   // 4K + 2K ns
    int64_t part_doubles = 0;           // nslab * rows * Nf
};
inline LombTermsPlan lomb_terms_plan(int64_t N, int64_t Nf, int64_t ns, long long nterms) {
    LombTermsPlan p;
    auto refuse = [&p](int status, const std::string &why) { p.status = status; p.why = why; return p; };
    if (nterms < 1 || nterms > kLombMaxTerms)
        return refuse(kLombTermsArgument, "lombscargle: nterms must be 1 .. " + std::to_string(kLombMaxTerms) + ", got " + std::to_string(nterms));
    if (N < 1 || Nf < 1 || ns < 1 || ns > kLombTermsMaxSignals)
        return refuse(kLombTermsArgument, "need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = " + std::to_string(N) + ", Nf = " + std::to_string(Nf) + ", ns = " +
                                              std::to_string(ns) + ")");
    if (Nf > kLombTermsMaxFreqs) return refuse(kLombTermsUnsupported, std::to_string(Nf) + " frequencies are too many");
    p.K = (int)nterms;
    p.ts = lomb_terms_ts(p.K, ns);
    p.acc = lomb_terms_acc(p.K, p.ts);
    p.sblocks = (int)ceil_div(ns, p.ts);
    p.rows = lomb_terms_rows(p.K, ns);
    const LombTiling tl = lomb_tiling(N, Nf, ns);
    p.ftiles = tl.ftiles; p.slab_samples = tl.slab_samples; p.nslab = tl.nslab;
    // one-dimensional grids of 256 threads (the slab sum) and of kLombTermsEpilogueBlock threads (the epilogue, ns in the second dimension)
    if ((double)p.rows * (double)Nf > 255.0 * (double)kLombMaxGrid)
        return refuse(kLombTermsUnsupported, "lombscargle: " + std::to_string(p.rows) + " rows of sums (nterms = " + std::to_string(nterms) + ", " +
                                                 std::to_string(ns) + " signals) of " + std::to_string(Nf) + " frequencies are more than one call takes");
    p.part_doubles = p.nslab * p.rows * Nf;
    return p;
}

}  // namespace lpvs
