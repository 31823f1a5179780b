// bls_plan.h -- the host-side decisions of the box least squares periodogram (bls: bls.hip, api.hip; include/lpvspectral.h g9; DESIGN.md
// 4.17): the checks of the host arguments, the quantisation of the weights and of the centred samples to 64-bit integers, the frequencies
// a workgroup folds from one staged block of samples (F), the signals of a pass (TS), the LDS bytes, the passes and the boxes tried.
// Pure functions of numbers: api.hip and bls.hip allocate and launch what they say and compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_bls_plan.py) compiles it as it is.
//
// QUANTISATION.  With w_n = W_n / sum W and wy_n = w_n (y_n - ybar) as launch_lomb_moments leaves them (doubles),
//     qw_n = rint(w_n 2^60),        qy_n = rint(wy_n 2^shy),    shy = 61 - L - (ilogb(A) + 1),   L = ceil(log2 N),  A = max_n |wy_n| > 0.
// NO SUM OF ANY SUBSET LEAVES 63 BITS.  |wy_n| <= A < 2^(ilogb(A) + 1), so |wy_n| 2^shy < 2^(61 - L) and |qy_n| <= 2^(61 - L) (rint is
// monotone and 2^(61 - L) an integer).  A subset has at most N <= 2^L terms: |sum| <= 2^61.  The search also forms S - s of two such
// sums (the samples outside a box: itself a subset sum) -- every value it holds is a subset sum, at most 2^61 < 2^63 in magnitude.
// The weights: w_n <= (1 + (N + 16) u) W_n / sum W (the device's sum W is a tree sum of N terms), so a subset's weights sum to less than
// 1 + 2^-20 for N <= 2^30, its integers to less than 2^60 (1 + 2^-20) + N / 2 < 2^61.  The product s (R - r) of the exact comparison of
// dips_only is below 2^122 and is taken in 128 bits.
// UNIT WEIGHTS (W == NULL): the weight of a box is its integer count at the scale 1 / N; no weight is quantised and no weight histogram
// is kept.  The centred samples are quantised as above (their w_n is the double 1 / N).
//
// THE OBJECTIVE, in double from the integers.  r, s: the integer sums of a box, R, S those of the whole histogram (NOT assumed to be 2^60
// and 0), rc = R - r, sc = S - s taken in integers.  Each is converted to double ONCE (round to nearest):
//     dq = (s s) / r + (sc sc) / rc - (S S) / R          evaluated as written: ((s * s) / r + (sc * sc) / rc) - (S * S) / R
// and only the result is scaled by the powers of two: Delta = dq 2^(60 - 2 shy) (weights), Delta = (dq N) 2^(-2 shy) (unit weights: one
// more rounding, of the product with N).  The largest dq wins; ties go to the smaller width, then to the smaller start.  Of the best box:
//     rd, rcd = r 2^-60, rc 2^-60 (weights) or count / N, (N - count) / N (unit weights: one division each),
//     depth = (sc / rcd - s / rd) 2^-shy,      depth_err = sqrt((1 / rd + 1 / rcd) / sum W),
//     power = min(1, max(Delta, 0) / YY) (standard; YY: below, order-free) or sum W max(Delta, 0) (chi2).
// dips_only keeps the boxes with s / r < sc / rc, decided exactly as s rc < sc r in 128-bit integers.
//
// WHAT THE RESULT MEANS.  Up to those roundings -- the conversions (5), three quotients, three products, two sums, the scaling by N, the
// quotient by YY: about a dozen, each 2^-53 of its operand -- the device returns the EXACT box least squares of the record whose w_n and
// w_n (y_n - ybar) are rounded to the quanta 2^-60 and 2^-shy <= A 2^-(60 - L): a sum of n terms is off by at most n / 2 quanta, whatever
// the order of the additions (they are integer additions).  For N = 2^20: the quantum of wy is at most A 2^-40, a sum over the whole
// record is off by at most 2^19 quanta = A 2^-21 -- 2^-41 of the N A such a sum can reach; the weights of a box are off by at most
// 2^19 2^-60 = 2^-41 of the total weight 1.
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "lomb_plan.h"

#if defined(__HIPCC__)
#define LPVS_BLS_HD __host__ __device__
#else
#define LPVS_BLS_HD
#endif

namespace lpvs {

enum { kBlsOk = 0, kBlsArgument = 1, kBlsUnsupported = 2 };

constexpr int kBlsMinBins = 8, kBlsMaxBins = 2048, kBlsWeightShift = 60;
constexpr int64_t kBlsMaxSamples = (int64_t)1 << 30, kBlsMaxFreqs = (int64_t)1 << 24;

// ---- the shifts ----------------------------------------------------------------------------------------------------------------------------
inline int bls_log2_ceil(int64_t N) {
    int L = 0;
    while (((int64_t)1 << L) < N) ++L;
    return L;
}
// A > 0 and finite (a subnormal A has its true exponent: ilogb); A = 0 is the constant signal and is never quantised
inline int bls_shift_y(double A, int64_t N) { return 61 - bls_log2_ceil(N) - (std::ilogb(A) + 1); }
// rint(v 2^shift): the scaling by scalbn is exact (|v 2^shift| <= 2^61, and a subnormal v only gains bits), rint rounds to nearest even
LPVS_BLS_HD inline long long bls_quantise(double v, int shift) { return (long long)rint(scalbn(v, shift)); }

// ---- YY, order-free ----------------------------------------------------------------------------------------------------------------------------
// YY_c = sum_n v_n, v_n = wy_n (y_n - ybar) >= 0 -- the terms launch_lomb_moments adds in a tree, whose bits depend on the order of the
// samples.  Here every term is cut into two integer words against the largest term M = max_n v_n, with sv = 61 - L - (ilogb(M) + 1):
//     x = v 2^sv (exact),   hi = rint(x) <= 2^(61 - L),   lo = rint((x - hi) 2^(61 - L)),  |lo| <= 2^(60 - L)   (x - hi is exact: |x - hi| <= 1/2
// and a multiple of ulp(x)); both words are added as integers (sums at most 2^61 and 2^60: no overflow, any order), and
//     YY = hi_sum 2^-sv + lo_sum 2^-(sv + 61 - L)        (two conversions, one addition: a function of the integers alone).
// What is dropped is at most half a unit of lo per term: N / 2 2^-(61 - L) 2^-sv <= M 2^(3 L - 122) in all -- 2^-62 of YY at N = 2^20, below
// 2^-53 of it up to N = 2^23 -- so YY is the sum of the rounded terms to within two roundings, closer to it than the tree sum.
constexpr int32_t kBlsNoShift = INT_MIN;   // (no term: a zero signal -- or terms that are not finite: the variance overflows)
LPVS_BLS_HD inline void bls_yy_words(double v, int sv, int log2n, long long *hi, long long *lo) {
    const double x = scalbn(v, sv), h = rint(x);
    *hi = (long long)h;
    *lo = (long long)rint(scalbn(x - h, 61 - log2n));
}
LPVS_BLS_HD inline double bls_yy(long long hi, long long lo, int sv, int log2n) { return scalbn((double)hi, -sv) + scalbn((double)lo, -(sv + 61 - log2n)); }

// ---- frequencies per workgroup, signals per pass ----------------------------------------------------------------------------------------------
// A workgroup keeps, per frequency, one 64-bit histogram per signal of the pass, one for the weights (not with unit weights) and the
// 32-bit counts:  LDS = F nbins ((ts + weighted) 8 + 4) bytes, at most kBlsLdsBudget = 63 KiB (1 KiB is left to the arg-max), so that two
// workgroups fit the 160 KiB of a CU whatever the shape.  ts: 1, 2 or 4 signals (the smallest that holds ns, at most 4), halved while one
// frequency does not fit.  F: 4, halved while the histograms do not fit or while fewer than kBlsFillWorkgroups = 256 workgroups (one per
// CU) would be left: every frequency of a workgroup is folded from the same staged samples, which pays only once the chip is full.
constexpr int kBlsLdsBudget = 63 * 1024, kBlsFillWorkgroups = 256, kBlsMaxF = 4, kBlsMaxTS = 4;
inline int64_t bls_lds_bytes(int F, int ts, bool unit, int nbins) { return (int64_t)F * nbins * ((ts + (unit ? 0 : 1)) * 8 + 4); }

struct BlsPlan {
    int status = kBlsArgument;
    std::string why;                    // (refused: the reason)
    int F = 0, ts = 0, passes = 0, unit = 0, log2n = 0;
    int64_t lds_bytes = 0, workgroups = 0;
    double boxes = 0;                   // sum over the frequencies of nbins (kmax - kmin + 1): the boxes tried per signal
};
inline BlsPlan bls_plan(int64_t N, int64_t ns, const double *f, int64_t Nf, int64_t nbins, const int32_t *kmin, const int32_t *kmax, int64_t min_count, bool unit,
                        int normalization) {
    BlsPlan p;
    auto refuse = [&p](int status, const std::string &why) { p.status = status; p.why = why; return p; };
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (N < 1 || Nf < 1 || ns < 1 || ns > 65535)
        return refuse(kBlsArgument, "bls: need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = " + ll(N) + ", Nf = " + ll(Nf) + ", ns = " + ll(ns) + ")");
    if (N > kBlsMaxSamples) return refuse(kBlsUnsupported, "bls: " + ll(N) + " samples are more than 2^30");
    if (Nf > kBlsMaxFreqs) return refuse(kBlsUnsupported, "bls: " + ll(Nf) + " frequencies are more than 2^24");
    if (nbins < kBlsMinBins || nbins > kBlsMaxBins) return refuse(kBlsArgument, "bls: nbins must lie in 8 .. 2048, got " + ll(nbins));
    if (min_count < 1) return refuse(kBlsArgument, "bls: min_count must be at least 1, got " + ll(min_count));
    if (normalization != 0 && normalization != 1) return refuse(kBlsArgument, "bls: normalization must be 0 (standard) or 1 (chi2), got " + ll(normalization));
    for (int64_t k = 0; k < Nf; ++k) {
        if (!std::isfinite(f[k])) return refuse(kBlsArgument, "bls: a frequency is not finite");
        if (!(f[k] > 0.0)) return refuse(kBlsArgument, "bls: frequency " + ll(k) + " is not positive");
        if (kmin[k] < 1) return refuse(kBlsArgument, "bls: kmin of frequency " + ll(k) + " is " + ll(kmin[k]) + ", below 1");
        if (kmin[k] > kmax[k]) return refuse(kBlsArgument, "bls: kmin of frequency " + ll(k) + " is " + ll(kmin[k]) + ", above its kmax " + ll(kmax[k]));
        if (kmax[k] > nbins / 2)
            return refuse(kBlsArgument, "bls: kmax of frequency " + ll(k) + " is " + ll(kmax[k]) + ", above nbins / 2 = " + ll(nbins / 2));
        p.boxes += (double)nbins * (double)(kmax[k] - kmin[k] + 1);
    }
    p.unit = unit ? 1 : 0;
    p.log2n = bls_log2_ceil(N);
    p.ts = ns <= 1 ? 1 : ns == 2 ? 2 : kBlsMaxTS;
    while (p.ts > 1 && bls_lds_bytes(1, p.ts, unit, (int)nbins) > kBlsLdsBudget) p.ts >>= 1;
    p.F = kBlsMaxF;
    while (p.F > 1 && (bls_lds_bytes(p.F, p.ts, unit, (int)nbins) > kBlsLdsBudget || ceil_div(Nf, p.F) < kBlsFillWorkgroups)) p.F >>= 1;
    p.lds_bytes = bls_lds_bytes(p.F, p.ts, unit, (int)nbins);
    p.passes = (int)ceil_div(ns, p.ts);
    p.workgroups = ceil_div(Nf, p.F);
    p.status = kBlsOk;
    return p;
}

}  // namespace lpvs
