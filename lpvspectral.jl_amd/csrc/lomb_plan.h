// lomb_plan.h -- the host-side decisions of the generalised Lomb-Scargle periodogram (lombscargle: lomb.hip, api.hip):
// whether a frequency grid is admitted to the transform path, how a long grid is cut into blocks of modes that fit the LDS-resident fine
// grid, how many real weight vectors a block transforms, how signals are grouped, which path `auto` takes, how the direct path tiles
// frequencies, signals and samples, and how many partial sums the fixed-order reductions leave.
// Pure functions of numbers: api.hip and lomb.hip allocate and launch what they say and compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_lomb_plan.py) compiles it as it is.
#pragma once

#include <string>

#include "gram_form_plan.h"

namespace lpvs {

// ---- admission -----------------------------------------------------------------------------------------------------------------------------
// f_k = a + k D + eps_k in cycles per unit of t.  make_ap_slots decides whether the grid is a progression up to rounding; it is given
// 2 pi max|t| for max|x|, so that its bound max|eps| max|x| <= kApMaxResidualPhase is a bound on the residual PHASE in radians as it is
// for the structured Gram (whose frequencies are angular).  Residuals are NOT refused: an admitted grid with eps_k != 0 takes the
// first-order term  sum W e^{i 2 pi (f + eps) t} = Z + i 2 pi eps Zt,  Zt = sum t W e^{i 2 pi f t}  (the x-weighted twin grids the spreading
// forms anyway), as the structured Gram and predict do.  What is applied are the residuals against a BLOCK's base (below), up to twice the
// admitted ones, and family 2 takes them twice over: the residual phase is at most 2e-7 (family 1) and 4e-7 (family 2), the dropped
// second-order term (phase^2 / 2) at most 2e-14 and 8e-14 of sum|W| -- below the spreading's own 1e-12.
// A grid of one frequency or of step 0 has no progression to speak of.
struct LombGrid {
    bool ok = false;            // the transform path may run
    bool twin = false;          // some eps_k != 0: the first-order term is applied
    double emax = 0;            // max|eps_k| against the end-point progression
    double a = 0;               // first frequency (exact: it is f[0])
    double D = 0;               // the step in cycles, rounded (reporting; the transforms use the angular steps below)
    double w1_hi = 0, w1_lo = 0;   // 2 pi D   in double-double: the angular step of family 1
    double w2_hi = 0, w2_lo = 0;   // 2 pi 2D: the angular step of family 2
    DD Dd;                      // the step in cycles, double-double
};
// 2 pi in double-double (the next term is -6e-33)
constexpr double kTwoPiHi = 6.283185307179586, kTwoPiLo = 2.4492935982947064e-16;
inline DD dd_times_two_pi(DD a) {
    const double p = a.hi * kTwoPiHi;
    if (!std::isfinite(p)) return DD{p, 0.0};
    return dd_fast_sum(p, std::fma(a.hi, kTwoPiHi, -p) + (a.hi * kTwoPiLo + a.lo * kTwoPiHi));
}
inline LombGrid lomb_admit(const std::vector<double> &f, double tam) {
    LombGrid g;
    if (f.size() < 2) return g;
    const ApSlots sl = make_ap_slots(f, 6.283185307179586 * tam, false);
    g.emax = sl.emax;
    const DD D = dd_div(dd_sum(f.back(), -f.front()), (double)(f.size() - 1));       // as make_ap_slots forms it
    if (!sl.ok || !(D.hi != 0.0) || !std::isfinite(D.hi)) return g;
    const DD w1 = dd_times_two_pi(D), w2 = dd_mul(w1, 2.0);
    g.w1_hi = w1.hi; g.w1_lo = w1.lo; g.w2_hi = w2.hi; g.w2_lo = w2.lo;
    g.a = f[0]; g.D = D.hi; g.Dd = D;
    for (double e : sl.eps) g.twin = g.twin || e != 0.0;
    g.ok = true;
    return g;
}

// ---- the cut into blocks -------------------------------------------------------------------------------------------------------------------
// One LDS-resident transform covers the modes 0 .. L-1 of one step: L is the largest count whose fine grid is within kNufftMaxGrid (2100).
// Block b holds the frequencies k0 .. k0 + count - 1; its transforms are
//   family 1 (C, S, YC, YS):  modes j of step D   after the weights were multiplied by e^{i 2 pi base t},  base  = f[k0]   (= a + k0 D + eps_k0)
//   family 2 (C2, S2):        modes j of step 2D  ...                                                       base2 = 2 f[k0]
// The base is a frequency of the grid itself, a double, so the pre-phase is that of the exact product base * t (an error-free product in
// the kernel, as the direct path forms every phase); what is left of a frequency inside its block,
//   eps'_j = f[k0 + j] - f[k0] - j D   (double-double, as the step itself: gram_form_plan.h says why long double is not enough),
// joins the first-order term (family 2: 2 eps'_j).  A block whose base is 0 needs no pre-phase; every block of a family shares one fine
// grid (that of the longest block), so the sample coordinates are computed once per family.
inline int lomb_max_block() {
    int L = (int)((double)kNufftMaxGrid / kNufftOversampling);
    while (nufft_grid_size(L + 1) <= kNufftMaxGrid) ++L;
    while (L > 1 && nufft_grid_size(L) > kNufftMaxGrid) --L;
    return L;
}
// LPVS_LOMB_BLOCK=L (experiment knob, read by api.hip through experiment_env): shorter blocks, so that tests cross block boundaries at
// small Nf.  Values outside 1 .. lomb_max_block() are ignored.
inline int lomb_block_len(long long knob) {
    const int L = lomb_max_block();
    return knob >= 1 && knob < L ? (int)knob : L;
}
struct LombBlock {
    int64_t k0 = 0;
    int count = 0;
    double base = 0;            // f[k0]; family 2 uses 2 * base (exact)
    bool prephase = false;      // base != 0
};
inline std::vector<LombBlock> lomb_blocks(const std::vector<double> &f, int L) {
    std::vector<LombBlock> bl;
    const int64_t Nf = (int64_t)f.size();
    for (int64_t k0 = 0; k0 < Nf; k0 += L) {
        LombBlock b;
        b.k0 = k0; b.count = (int)(Nf - k0 < L ? Nf - k0 : L);
        b.base = f[(size_t)k0]; b.prephase = b.base != 0.0;
        bl.push_back(b);
    }
    return bl;
}
// residuals of the frequencies against their block's base and the step
inline std::vector<double> lomb_block_residuals(const std::vector<double> &f, const LombGrid &g, int L) {
    std::vector<double> e(f.size());
    for (size_t k = 0; k < f.size(); ++k) {
        const size_t k0 = k / (size_t)L * (size_t)L;
        e[k] = dd_sub(dd_sum(f[k], -f[k0]), dd_mul(g.Dd, (double)(k - k0))).hi;
    }
    return e;
}
// fine grid of a family: that of its longest block
inline int lomb_fine_grid(int64_t Nf, int L) { return nufft_grid_size(Nf < L ? Nf : L); }

// real weight vectors of one transform: family 1 carries w and w y_c of the group's signals, family 2 only w; a pre-phased block's
// weights are complex, and the transform of a complex weight is the sum of the transforms of its real and imaginary parts: twice as many.
inline int lomb_weight_vectors(int family, int group_signals, bool prephase) { return (family == 1 ? 1 + group_signals : 1) * (prephase ? 2 : 1); }
// signals per transform: with the pre-phase 2 (1 + g) <= kNufftMaxWeights; more signals go in further groups (each carries w again)
constexpr int kLombGroupSignals = (int)(kNufftMaxWeights / 2) - 1;       // 127
inline int64_t lomb_signal_groups(int64_t ns) { return ceil_div(ns, kLombGroupSignals); }

// ---- the path ------------------------------------------------------------------------------------------------------------------------------
enum { kLombPathAuto = 0, kLombPathDirect = 1, kLombPathNufft = 2, kLombPathRefused = -1 };
// `auto` takes the transforms when the grid is admitted AND all three hold: N >= kLombNufftMinSamples, Nf >= kLombNufftMinFreqs and
// N Nf >= kLombNufftMinWork.  Measured (profiles/lomb_time.txt, one signal, device time of the whole call): the direct kernel does one
// sincospi per (sample, frequency) and little else, 2.4e-9 ms each, so the transforms' fixed cost -- about 0.4 ms per transform, two
// per block -- is only won back on long records.
//   samples: NOT kNufftMinSamples (4096) but 2^18.  At Nf = 512 the direct path is ahead at every N up to 2^19 (0.87 against 0.92 ms;
//            0.20 against 0.51 ms at 2^12); a grid of four blocks (Nf = 8192) is still 2.4 times behind at N = 2^16.
//   frequencies: at N = 2^20 the transforms are 9, 3.0 and 1.4 times BEHIND at Nf = 64, 128 and 256 (short grids have small fine grids,
//            whose cells many samples share) and 1.4 times ahead at 512.
//   work:    at Nf = 2048 the crossover lies between N = 2^17 (0.80 against 1.09 ms) and 2^18 (1.42 against 1.11 ms), at Nf = 512 between
//            2^19 and 2^20: N Nf = 2^29 on both lines.
// Every measured row's faster path is the one this rule takes; at N = 2^20 the transforms are 4.2 times ahead at Nf = 4096 and 3.1
// times at 65536 (32 blocks).
constexpr int64_t kLombNufftMinSamples = (int64_t)1 << 18, kLombNufftMinFreqs = 512, kLombNufftMinWork = (int64_t)1 << 29;
inline bool lomb_transforms_pay(int64_t N, int64_t Nf) {
    return N >= kLombNufftMinSamples && Nf >= kLombNufftMinFreqs && N * Nf >= kLombNufftMinWork;   // (Nf <= 2^24, N < 2^39: no overflow)
}
// does the call have to look at the grid at all (max|t| is a device reduction, the admission walks the grid)?  Only when the transforms were
// asked for, or `auto` could take them
inline bool lomb_needs_admission(int requested, int64_t N, int64_t Nf) {
    return requested == kLombPathNufft || (requested == kLombPathAuto && lomb_transforms_pay(N, Nf));
}
inline int lomb_choose_path(int requested, bool grid_ok, int64_t N, int64_t Nf) {
    if (requested == kLombPathDirect) return kLombPathDirect;
    if (requested == kLombPathNufft) return grid_ok ? kLombPathNufft : kLombPathRefused;
    if (requested != kLombPathAuto) return kLombPathRefused;
    return grid_ok && lomb_transforms_pay(N, Nf) ? kLombPathNufft : kLombPathDirect;
}

// ---- the direct path -----------------------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads = kLombFreqTile frequencies x kLombSampleLanes sample lanes (one wave per lane: the staged sample is an LDS
// broadcast) owns a tile of frequencies, a block of ts signals (ts in {1, 4}: 4 + 2 ts accumulators per thread) and one slab of samples,
// which it stages through LDS kLombStage at a time.  The slabs are cut so that (tiles x slabs) is about kLombWorkgroups, never below
// kLombMinSlab samples; nothing here depends on the number of signals, so a column of a multi-signal call sees the sums of its own call.
constexpr int kLombFreqTile = 64, kLombSampleLanes = 4, kLombStage = 256;
constexpr int64_t kLombWorkgroups = 2048, kLombMinSlab = 1024, kLombMaxSlabs = 1024;
struct LombTiling { int ts = 0, sblocks = 0, acc = 0; int64_t ftiles = 0, slab_samples = 0, nslab = 0; };
inline LombTiling lomb_tiling(int64_t N, int64_t Nf, int64_t ns) {
    LombTiling t;
    t.ts = ns <= 1 ? 1 : 4;
    t.sblocks = (int)ceil_div(ns, t.ts);
    t.acc = 4 + 2 * t.ts;
    t.ftiles = ceil_div(Nf, kLombFreqTile);
    int64_t want = ceil_div(kLombWorkgroups, t.ftiles);
    const int64_t most = ceil_div(N, kLombMinSlab);
    if (want > most) want = most;
    if (want > kLombMaxSlabs) want = kLombMaxSlabs;
    if (want < 1) want = 1;
    t.slab_samples = round_up(ceil_div(N, want), kLombStage);
    t.nslab = ceil_div(N, t.slab_samples);
    return t;
}
// the moments (sum W, the weighted means, YY): every workgroup of kLombSumBlock samples leaves one partial (a pairwise tree over its
// threads); one workgroup per row then adds the slabs: thread t the slabs t, t + 256, ... in ascending order, then the same tree
constexpr int kLombSumBlock = 256;
inline int64_t lomb_sum_slabs(int64_t N) { return ceil_div(N, kLombSumBlock); }

// ---- constant signals ----------------------------------------------------------------------------------------------------------------------
// The standard power is p / YY, and 0 for a constant signal.  In floating point a constant signal's YY is a rounding residue, so the rule is
// YY <= lomb_yy_noise(..) -> 0, with the noise worked from how YY was formed (u = 2^-53; R = sum w y^2 of the signal as given):
//   centred data: the device's weighted mean is off by at most (N + 16) u sum w|y| <= (N + 16) u sqrt(R), and every centred sample with it:
//                 YY carries up to ((N + 16) u)^2 R of it;
//   fit_mean:     YY - Y^2 subtracts two sums of N terms with Y^2 <= YY: up to 3 (N + 16) u YY (YY before the subtraction).
// Neither: YY = R, which is 0 only for the zero signal.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline double lomb_yy_noise(double N, bool center, bool fit_mean, double R, double YY_before) {
    const double nu = (N + 16.0) * 0x1p-53;
    return (center ? nu * nu * R : 0.0) + (fit_mean ? 3.0 * nu * YY_before : 0.0);
}

// ---- the degenerate rule -------------------------------------------------------------------------------------------------------------------
// D <= kLombDegenerate (CC + SS)^2, with CC + SS taken BEFORE the floating-mean terms are subtracted (it is 1 there; after the
// subtraction it is itself rounding noise at f = 0, where the rule has to bite)
constexpr double kLombDegenerate = 0x1p-40;

// ---- windows (lombscargle_spectrogram / lombscargle_welch: include/lpvspectral.h g5) --------------------------------------
// Every window is a g4 estimate of its own samples; one call runs them all through segmented kernels.  Only the direct path: the
// transforms pay from kLombNufftMinSamples = 2^18 samples per transform on, and windows are far shorter.
// The samples of a window are cut into slabs of kLombWindowSlab -- a CONSTANT (a multiple of kLombStage, at least kLombMinSlab), not a
// function of the call as lomb_tiling's slab is: a window's slabs, and with them the order of every addition behind its column, depend on
// its own count alone, so the column has the same bits whether the window is computed alone, among others or in another place of the list.
// The work list holds one item per (window, slab); empty windows leave none.  The moments' kernels take one item per workgroup (its
// blocks of kLombSumBlock samples in ascending order), the direct kernel one item, one tile of frequencies and one block of signals;
// a window's items are then added in the pairwise tree of lomb_slab_sum_kernel.
constexpr int64_t kLombWindowSlab = 1024, kLombMaxWindows = (int64_t)1 << 24;
static_assert(kLombWindowSlab % kLombStage == 0 && kLombWindowSlab >= kLombMinSlab && kLombWindowSlab % kLombSumBlock == 0, "the slab of a window");
struct LombWindowItem {
    int32_t window = 0, slab = 0;       // the window, and the index of this slab within it
    int64_t first = 0, last = 0;        // its samples first .. last (inclusive), counted from the window's first sample
};
struct LombWindowPlan {
    bool ok = false;
    std::string why;                    // (refused: the reason)
    int64_t slab_samples = kLombWindowSlab;
    std::vector<LombWindowItem> items;
    std::vector<int32_t> nslab;         // per window: its slabs (0: an empty window)
    std::vector<int64_t> offset;        // per window: the index of its first item; one more entry: the number of items
};
inline LombWindowPlan lomb_window_plan(const std::vector<int64_t> &counts) {
    LombWindowPlan p;
    if ((int64_t)counts.size() > kLombMaxWindows) {
        p.why = "lombscargle: " + std::to_string(counts.size()) + " windows are more than 2^24";
        return p;
    }
    p.nslab.reserve(counts.size()); p.offset.reserve(counts.size() + 1);
    for (size_t w = 0; w < counts.size(); ++w) {
        const int64_t n = counts[w];
        if (n < 0) { p.why = "lombscargle: window " + std::to_string(w) + " has a negative count"; return p; }
        const int64_t ns = ceil_div(n, kLombWindowSlab);
        if (ns > kLombMaxSlabs) {
            p.why = "lombscargle: window " + std::to_string(w) + " holds " + std::to_string(n) + " samples, more than the " +
                    std::to_string(kLombMaxSlabs * kLombWindowSlab) + " a window may hold (" + std::to_string(kLombMaxSlabs) + " slabs of " +
                    std::to_string(kLombWindowSlab) + ")";
            return p;
        }
        p.offset.push_back((int64_t)p.items.size());
        p.nslab.push_back((int32_t)ns);
        for (int64_t s = 0; s < ns; ++s) {
            LombWindowItem it;
            it.window = (int32_t)w; it.slab = (int32_t)s;
            it.first = s * kLombWindowSlab;
            it.last = (it.first + kLombWindowSlab < n ? it.first + kLombWindowSlab : n) - 1;
            p.items.push_back(it);
        }
    }
    p.offset.push_back((int64_t)p.items.size());
    p.ok = true;
    return p;
}
// the direct kernel's tiles of frequencies and blocks of signals (as lomb_tiling's; the slab is the constant)
inline LombTiling lomb_windows_tiling(int64_t Nf, int64_t ns) {
    LombTiling t;
    t.ts = ns <= 1 ? 1 : 4;
    t.sblocks = (int)ceil_div(ns, t.ts);
    t.acc = 4 + 2 * t.ts;
    t.ftiles = ceil_div(Nf, kLombFreqTile);
    t.slab_samples = kLombWindowSlab;
    return t;
}
// one-dimensional grids: (items x tiles) workgroups of the direct kernel, a thread per element of the trees and of the epilogue
constexpr int64_t kLombMaxGrid = ((int64_t)1 << 31) - 1;
inline bool lomb_windows_fit(int64_t nitems, int64_t nwin, int64_t Nf, int64_t ns) {
    const double most = (double)kLombMaxGrid, rows = (double)(4 + 2 * ns) * (double)Nf;   // (products of up to 2^65: compared as doubles)
    return (double)nitems * (double)ceil_div(Nf, kLombFreqTile) <= most && (double)nwin * rows <= 255.0 * most && (double)nitems * rows <= 255.0 * most;
}

}  // namespace lpvs
