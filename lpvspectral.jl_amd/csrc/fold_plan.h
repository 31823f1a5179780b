// fold_plan.h -- the host-side decisions of the fold statistics (pdm, aov, conditional_entropy: fold.hip, uneven.hip;
// include/lpvspectral.h g10): the checks of the host arguments, the frequencies a workgroup folds from one staged block of
// samples (F), the signals of a pass (TS), the private copies of the count histogram (copies), the LDS bytes, the passes and the
// workgroups.  Pure functions of numbers: uneven.hip and fold.hip allocate and launch what they say and compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_fold_plan.py) compiles it as it is.
//
// PDM / AOV.  The record is quantised exactly as bls_plan.h says (qw_n = rint(w_n 2^60), qy_n = rint(wy_n 2^shy); with W == NULL the weight
// of a bin is its count at the scale 1 / N) and folded by bls's fold into nfine = nbins covers fine bins.  Coarse bin m, 0 <= m < nfine, is
// the covers adjacent fine bins m .. m + covers - 1, wrapping; r_m, s_m: its integer sums (subset sums: bls_plan.h bounds them by 2^61);
// R, S: the integer totals of the histograms.  Each integer is converted to double ONCE (round to nearest):
//     term_m = (s_m * s_m) / r_m   where r_m > 0, else no term,
//     sb     = (sum_m term_m) / covers - (S * S) / R                              evaluated as written,
// and only the result is scaled by the powers of two: SB = sb 2^(60 - 2 shy) (weights) or (sb N) 2^(-2 shy) (W == NULL: one more
// rounding, of the product with N); explained = min(1, max(SB, 0) / YY), YY: bls's order-free sum (bls_plan.h: bls_yy).
// THE ORDER OF THE SUM.  Thread tid of the 256 adds the terms of its coarse bins m = tid, tid + 256, ... in ascending order to one
// accumulator that starts at 0 (a bin without a term adds nothing); the 64 accumulators of a wave are added in a tree -- lane l takes
// lane l + 32, then l + 16, 8, 4, 2, 1 --; the four wave sums W0 .. W3 are added as (W0 + W1) + (W2 + W3).  At most
// ceil(nfine / 256) + 8 additions lie on any path, all of non-negative terms.
// M = #{m : r_m > 0} is a property of the fold alone, shared by the signals.  DEGENERATE: a constant signal (A_c = 0, a YY within
// lomb_yy_noise or one that is not finite -- bls's rule), M <= covers (everything in one run of fine bins: no between-bin variance is
// defined), covers N <= M (no degree of freedom is left within the bins), or an SB that is not finite: explained = 0, flagged, counted.
//
// CONDITIONAL ENTROPY.  Unweighted by definition.  ymin, ymax per signal by integer atomic minima / maxima of an order-preserving key of
// the double (order-free, exact); den = ymax - ymin, and per sample u = (y - ymin) / den, j = min(mbins - 1, (int)floor(u mbins)), stored
// once as a byte; den == 0 or not finite: every j = 0, the signal is flagged degenerate and its entropy is 0.  The fold is bls's, into
// nbins phase bins; n_ij: the 32-bit counts, n_i their row sums (integers).  The entropy, in double from the integers:
//     term_ij = n_ij * log(n_i / n_ij)    where n_ij > 0 (each integer converted once; one quotient, one log, one product; term >= 0),
//     H = (sum_ij term_ij) / N.
// THE ORDER OF THE SUM.  Thread tid adds the terms of its cells q = i mbins + j = tid, tid + 256, ... in ascending order; then the same
// tree over the wave and the same (W0 + W1) + (W2 + W3): at most ceil(nbins mbins / 256) + 8 additions on any path.
// COPIES.  The counts of one (frequency, signal) may be kept in 1, 2 or 4 private copies, wave v adding to copy v mod copies, merged by
// integer additions before the row sums: the result is the same for every value.  The plan takes ONE.  Measured (profiles/fold_time.txt,
// MI355X, 10 x 5 cells, where a wave's 64 samples share 50 addresses): 1, 2 and 4 copies are within 2 % of each other at every shape
// with no consistent winner (9.49, 9.49, 9.43 ms at N = 2^18, Nf = 65536; repeats of one configuration differ by up to 5 %) -- the
// conflicts that cost are those WITHIN a wave, which copies per wave do not remove.  LPVS_CENT_COPIES (an experiment knob) asks for 1, 2
// or 4, halved while the LDS does not hold them, so that the comparison can be repeated.
//
// WHAT THE RESULTS MEAN.  pdm: up to the counted roundings -- per term two conversions, a product and a quotient; the additions above;
// the division by covers; S S / R (three conversions, two operations); the subtraction; the scaling by N; the quotient by YY -- the device
// returns the exact statistic of the record whose w_n and w_n (y_n - ybar) are rounded to the quanta 2^-60 and 2^-shy: a sum of n terms
// is off by at most n / 2 quanta, whatever the order.  cent: the counts are exact; H carries per term the quotient, the log (the device's,
// within 2 ulp) and the product, then the additions and the division by N.  log(x (1 + d)) moves by d whatever x is, so the error of a
// term is absolute in n_ij d: the bound on H is c 2^-53 (1 + H), not relative to H.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "bls_plan.h"

namespace lpvs {

enum { kFoldOk = 0, kFoldArgument = 1, kFoldUnsupported = 2 };

constexpr int kPdmMaxFine = 2048;
constexpr int kCentMaxBins = 256, kCentMaxValueBins = 64, kCentMaxCells = 8192;

// the checks both entries share; who: "pdm" or "conditional_entropy"
inline bool fold_check_common(const char *who_, int64_t N, int64_t ns, const double *f, int64_t Nf, int *status, std::string *why) {
    const std::string who(who_);
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (N < 1 || Nf < 1 || ns < 1 || ns > 65535) {
        *status = kFoldArgument;
        *why = who + ": need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = " + ll(N) + ", Nf = " + ll(Nf) + ", ns = " + ll(ns) + ")";
        return false;
    }
    if (N > kBlsMaxSamples) { *status = kFoldUnsupported; *why = who + ": " + ll(N) + " samples are more than 2^30"; return false; }
    if (Nf > kBlsMaxFreqs) { *status = kFoldUnsupported; *why = who + ": " + ll(Nf) + " frequencies are more than 2^24"; return false; }
    return true;
}
inline bool fold_check_frequencies(const char *who_, const double *f, int64_t Nf, int *status, std::string *why) {
    const std::string who(who_);
    for (int64_t k = 0; k < Nf; ++k) {
        if (!std::isfinite(f[k])) { *status = kFoldArgument; *why = who + ": a frequency is not finite"; return false; }
        if (!(f[k] > 0.0)) { *status = kFoldArgument; *why = who + ": frequency " + std::to_string((long long)k) + " is not positive"; return false; }
    }
    return true;
}

// ---- pdm / aov: bls's histograms over nfine bins, bls's budget rule ------------------------------------------------------------------------------
struct PdmPlan {
    int status = kFoldArgument;
    std::string why;                    // (refused: the reason)
    int F = 0, ts = 0, passes = 0, unit = 0, log2n = 0, nfine = 0;
    int64_t lds_bytes = 0, workgroups = 0;
};
inline PdmPlan pdm_plan(int64_t N, int64_t ns, const double *f, int64_t Nf, int64_t nbins, int64_t covers, bool unit) {
    PdmPlan p;
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (!fold_check_common("pdm", N, ns, f, Nf, &p.status, &p.why)) return p;
    if (nbins < 2) { p.status = kFoldArgument; p.why = "pdm: nbins must be at least 2, got " + ll(nbins); return p; }
    if (covers < 1) { p.status = kFoldArgument; p.why = "pdm: covers must be at least 1, got " + ll(covers); return p; }
    if (nbins > kPdmMaxFine || covers > kPdmMaxFine || nbins * covers > kPdmMaxFine) {
        p.status = kFoldArgument;
        p.why = "pdm: nbins covers must lie in 2 .. 2048, got " + ll(nbins) + " x " + ll(covers);
        return p;
    }
    if (!fold_check_frequencies("pdm", f, Nf, &p.status, &p.why)) return p;
    p.nfine = (int)(nbins * covers);
    p.unit = unit ? 1 : 0;
    p.log2n = bls_log2_ceil(N);
    p.ts = ns <= 1 ? 1 : ns == 2 ? 2 : kBlsMaxTS;
    while (p.ts > 1 && bls_lds_bytes(1, p.ts, unit, p.nfine) > kBlsLdsBudget) p.ts >>= 1;
    p.F = kBlsMaxF;
    while (p.F > 1 && (bls_lds_bytes(p.F, p.ts, unit, p.nfine) > kBlsLdsBudget || ceil_div(Nf, p.F) < kBlsFillWorkgroups)) p.F >>= 1;
    p.lds_bytes = bls_lds_bytes(p.F, p.ts, unit, p.nfine);
    p.passes = (int)ceil_div(ns, p.ts);
    p.workgroups = ceil_div(Nf, p.F);
    p.status = kFoldOk;
    return p;
}

// ---- conditional entropy: 32-bit counts, private copies ----------------------------------------------------------------------------------------
inline int64_t cent_lds_bytes(int F, int copies, int ts, int cells) { return (int64_t)F * copies * ts * cells * 4; }

struct CentPlan {
    int status = kFoldArgument;
    std::string why;
    int F = 0, ts = 0, passes = 0, copies = 0, cells = 0;
    int64_t lds_bytes = 0, workgroups = 0;
};
// copies_knob: 0 (the rule: one copy) or the value of LPVS_CENT_COPIES; anything but 1, 2 and 4 is ignored
inline CentPlan cent_plan(int64_t N, int64_t ns, const double *f, int64_t Nf, int64_t nbins, int64_t mbins, int64_t copies_knob) {
    CentPlan p;
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (!fold_check_common("conditional_entropy", N, ns, f, Nf, &p.status, &p.why)) return p;
    if (nbins < 2 || nbins > kCentMaxBins) { p.status = kFoldArgument; p.why = "conditional_entropy: nbins must lie in 2 .. 256, got " + ll(nbins); return p; }
    if (mbins < 2 || mbins > kCentMaxValueBins) { p.status = kFoldArgument; p.why = "conditional_entropy: mbins must lie in 2 .. 64, got " + ll(mbins); return p; }
    if (nbins * mbins > kCentMaxCells) {
        p.status = kFoldArgument;
        p.why = "conditional_entropy: nbins mbins must be at most 8192, got " + ll(nbins) + " x " + ll(mbins);
        return p;
    }
    if (!fold_check_frequencies("conditional_entropy", f, Nf, &p.status, &p.why)) return p;
    p.cells = (int)(nbins * mbins);
    p.ts = ns <= 1 ? 1 : ns == 2 ? 2 : kBlsMaxTS;
    while (p.ts > 1 && cent_lds_bytes(1, 1, p.ts, p.cells) > kBlsLdsBudget) p.ts >>= 1;
    p.F = kBlsMaxF;
    while (p.F > 1 && (cent_lds_bytes(p.F, 1, p.ts, p.cells) > kBlsLdsBudget || ceil_div(Nf, p.F) < kBlsFillWorkgroups)) p.F >>= 1;
    p.copies = copies_knob == 2 || copies_knob == 4 ? (int)copies_knob : 1;
    while (p.copies > 1 && cent_lds_bytes(p.F, p.copies, p.ts, p.cells) > kBlsLdsBudget) p.copies >>= 1;
    p.lds_bytes = cent_lds_bytes(p.F, p.copies, p.ts, p.cells);
    p.passes = (int)ceil_div(ns, p.ts);
    p.workgroups = ceil_div(Nf, p.F);
    p.status = kFoldOk;
    return p;
}

// the order-preserving key of a double: keys compare as unsigned integers the way the doubles compare (no NaN reaches it: Record::check)
LPVS_BLS_HD inline unsigned long long fold_key(double v) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
LPVS_BLS_HD inline double fold_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    __builtin_memcpy(&v, &b, sizeof(v));
    return v;
}
// the value bin of y: den = ymax - ymin; a den that is 0 or not finite puts every sample into bin 0
LPVS_BLS_HD inline int cent_value_bin(double y, double ymin, double den, int mbins) {
    if (!(den > 0.0) || !(den < 1.0 / 0.0)) return 0;
    const double u = (y - ymin) / den;
    const int j = (int)floor(u * (double)mbins);
    return j < 0 ? 0 : j < mbins - 1 ? j : mbins - 1;
}

}  // namespace lpvs
