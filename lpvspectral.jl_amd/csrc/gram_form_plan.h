// gram_form_plan.h -- the host-side decisions at the front of every solve (api.hip's problem constructors and the window engine's
// choose_gram_form): whether a frequency grid is admitted to the structured Gram and with which slot tables, which
// Gram form runs, whether its slot sums go through the non-uniform FFT, how the dense forms tile and split their work, and what is
// reported as issued flops.  Pure functions of numbers: api.hip, nufft.hip and gram.hip allocate and launch what they say and compute
// none of this themselves.
// No HIP dependency: the host-side test (tests/test_gram_form_plan.py) compiles it as it is.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lpvspectral.h"

namespace lpvs {

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- small host rules --------------------------------------------------------------------------------------------------------------------
// 1: the zero frequency leads the grid; 0: there is none; -1: it sits elsewhere (an error)                      src/lsfft.jl:20-24
inline int64_t check_freq_host(const double *f, int64_t Nf) {
    for (int64_t i = 0; i < Nf; ++i)
        if (f[i] == 0.0) return i == 0 ? 1 : -1;
    return 0;
}

// basis centres (src/utilities.jl:24-32); twice-precision range reproduced with long double
inline void basis_centers(double lo, double hi, double amax, int64_t Nv, int coulomb, std::vector<double> &vc, double *gamma) {
    if (!coulomb) {
        vc.resize((size_t)Nv);
        for (int64_t j = 0; j < Nv; ++j)
            vc[j] = Nv > 1 ? (double)((long double)lo + (long double)j * ((long double)hi - (long double)lo) / (long double)(Nv - 1)) : lo;
        *gamma = (double)Nv / std::fabs(vc[0] - vc[Nv - 1]);
    } else {
        vc.resize((size_t)(2 * Nv));
        for (int64_t j = 0; j < Nv; ++j) {
            const double c = (double)((long double)(j + 1) * (long double)amax / (long double)(Nv + 1));
            vc[Nv + j] = c;
            vc[Nv - 1 - j] = -c;
        }
        *gamma = (double)(2 * Nv) / std::fabs(vc[0] - vc[2 * Nv - 1]);
    }
}

// ---- double-double arithmetic for the slot tables -------------------------------------------------------------------------------------------
// The tables hold frequencies as hi + lo (106 bits) because the kernels form the phase of the REAL product.  An 80-bit long double has 64:
// a table worked in it is off by up to 2^-64 |w| per operation, a phase error of 2^-64 |w x| -- 4e-13 rad at |w x| = 6e6 and 7e-12 at 9e7,
// measured in rational arithmetic (tests/test_phase_ref_host.py) -- so the tables are worked in double-double, with error-free sums and
// products (an inf or NaN keeps a zero low word, so that it travels as it does in plain arithmetic).
struct DD { double hi = 0, lo = 0; };
inline DD dd_fast_sum(double a, double b) {              // |a| >= |b| (or a == 0)
    const double s = a + b;
    return std::isfinite(s) ? DD{s, b - (s - a)} : DD{s, 0.0};
}
inline DD dd_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return std::isfinite(s) ? DD{s, (a - (s - bb)) + (b - bb)} : DD{s, 0.0};
}
inline DD dd_add(DD a, DD b) {
    DD s = dd_sum(a.hi, b.hi);
    const DD t = dd_sum(a.lo, b.lo);
    s = dd_fast_sum(s.hi, s.lo + t.hi);
    return dd_fast_sum(s.hi, s.lo + t.lo);
}
inline DD dd_sub(DD a, DD b) { return dd_add(a, DD{-b.hi, -b.lo}); }
inline DD dd_mul(DD a, double b) {
    const double p = a.hi * b;
    if (!std::isfinite(p)) return DD{p, 0.0};
    return dd_fast_sum(p, std::fma(a.lo, b, std::fma(a.hi, b, -p)));
}
inline DD dd_div(DD a, double b) {                       // three quotient digits: the remainder after each is exact to double-double
    const double q1 = a.hi / b;
    if (!std::isfinite(q1)) return DD{q1, 0.0};
    const DD r1 = dd_sub(a, dd_mul(DD{q1, 0.0}, b));
    const double q2 = r1.hi / b;
    const DD r2 = dd_sub(r1, dd_mul(DD{q2, 0.0}, b));
    const DD q = dd_fast_sum(q1, q2);
    return dd_fast_sum(q.hi, q.lo + r2.hi / b);
}

// ---- slot tables of the structured Gram (nudft.hip) ---------------------------------------------------------------------------------------
// For frequencies w_f = a + f*D + eps_f: progressions worked and held in double-double, each family padded to a multiple of 8:
//   [0, nf8): m*D (differences), [nf8, nf8+s8): 2a + s*D (sums); the right-hand side uses a + f*D, f < nf8.
// MERGED layout: when 2a is (up to rounding) an integer multiple j0 < Nf of D -- default_freqs (a = 0), the README grid
// w = D*(1..Nf) (a = D) -- the sum frequencies (j0 + s) D are multiples of D like the differences, so ONE progression
// j*D, j = 0 .. j0+2Nf-2 serves both families: 2Nf-1+j0 slots instead of 3Nf-1 (a third less work); the sum of (f, f') is
// slot s0 + f + f' with s0 = j0, and the rounding residual delta = 2a - j0*D joins the first-order correction.
struct ApStep { double hi[8], lo[8]; };   // b*D in double-double, b = 0..7 (in-group offsets of the slot progressions)
struct ApSlots {
    bool ok = false;
    double emax = 0;
    int64_t nf8 = 0, s8 = 0, nsl = 0;
    bool merged = false;   // one progression j*D serves differences and sums (see above)
    int64_t s0 = 0;        // slot of the sum frequency 2a (split layout: nf8; merged: j0)
    double delta = 0;      // merged layout: 2a - j0*D
    std::vector<double> eps, om_hi, om_lo, omr_hi, omr_lo;
    ApStep step{};
};
// admitted when max|eps_f| * max|x| is at most this: the dropped second-order term (eps x)^2/2 is then <= 5e-15.  The merged layout's
// residual delta is held to the same bound.
constexpr double kApMaxResidualPhase = 1e-7;
// Single-precision callers (_f32 entry points; f32_grid): the frequency grid is a progression rounded to FLOATS, so its residuals are
// up to 2^-24 |w| and |eps| max|x| reaches 0.2 rad at the cfg3 size -- far beyond the double-precision admission bound.  But a
// Float32 run of the reference evaluates fl32(w x) itself, a phase error of up to 2^-24 |w x|: snapping w to the exact
// progression its floats were rounded from stays inside that error.  Residuals up to 2^-23 max|w| (one float ulp) are admitted ...
constexpr double kApF32MaxRelResidual = 0x1p-23;
// ... and dropped when their phases exceed this: snapped grid, NO first-order term -- G is then exactly the Gram of the regressor at
// the snapped frequencies (positive semidefinite by construction), which a first-order expansion with |eps x| ~ 0.2 would not
// guarantee.  Smaller residual phases keep the first-order term (error (eps x)^2/2 <= 5e-6).
constexpr double kApF32KeepResidualPhase = 3e-3;

// (A NaN in w is dropped by fmax: emax stays what the other residuals give and the grid is admitted -- known, and pinned by the test.)
inline ApSlots make_ap_slots(const std::vector<double> &hw, double xam, bool f32_grid) {
    ApSlots sl;
    const int64_t Nf = (int64_t)hw.size();
    const DD a0{hw[0], 0.0}, D = Nf > 1 ? dd_div(dd_sum(hw[Nf - 1], -hw[0]), (double)(Nf - 1)) : DD{};
    sl.eps.resize((size_t)Nf);
    for (int64_t f = 0; f < Nf; ++f) {
        sl.eps[f] = dd_sub(DD{hw[f], 0.0}, dd_add(a0, dd_mul(D, (double)f))).hi;
        sl.emax = std::fmax(sl.emax, std::fabs(sl.eps[f]));
    }
    double wam = 0;
    for (double v : hw) wam = std::fmax(wam, std::fabs(v));
    sl.ok = std::isfinite(sl.emax) && std::isfinite(xam) && sl.emax * xam <= kApMaxResidualPhase;
    if (!sl.ok && f32_grid && std::isfinite(sl.emax) && std::isfinite(xam) && sl.emax <= kApF32MaxRelResidual * wam) {
        sl.ok = true;
        if (sl.emax * xam > kApF32KeepResidualPhase) for (auto &e : sl.eps) e = 0.0;
    }
    if (!sl.ok) return sl;
    sl.nf8 = round_up(Nf, 8); sl.s8 = round_up(2 * Nf - 1, 8); sl.nsl = sl.nf8 + sl.s8;
    auto split = [](DD v, double &hi, double &lo) { hi = v.hi; lo = v.lo; };
    const DD a2 = dd_mul(a0, 2.0);
    sl.omr_hi.resize((size_t)sl.nf8); sl.omr_lo.resize((size_t)sl.nf8);
    sl.s0 = sl.nf8;
    if (Nf > 1 && D.hi != 0.0) {
        const long double j0r = 2.0L * (long double)a0.hi / ((long double)D.hi + (long double)D.lo);
        const long long j0 = llroundl(j0r);
        const double delta = dd_sub(a2, dd_mul(D, (double)j0)).hi;
        if (j0 >= 0 && j0 < Nf && std::fabs(delta) * xam <= kApMaxResidualPhase) {
            sl.merged = true;
            sl.s0 = j0; sl.delta = delta;
            sl.nsl = round_up(j0 + 2 * Nf - 1, 8);
            sl.s8 = sl.nsl;
        }
    }
    sl.om_hi.resize((size_t)sl.nsl); sl.om_lo.resize((size_t)sl.nsl);
    if (sl.merged) {
        for (int64_t j = 0; j < sl.nsl; ++j) split(dd_mul(D, (double)j), sl.om_hi[j], sl.om_lo[j]);
    } else {
        for (int64_t m = 0; m < sl.nf8; ++m) split(dd_mul(D, (double)m), sl.om_hi[m], sl.om_lo[m]);
        for (int64_t q = 0; q < sl.s8; ++q) split(dd_add(a2, dd_mul(D, (double)q)), sl.om_hi[sl.nf8 + q], sl.om_lo[sl.nf8 + q]);
    }
    for (int64_t f = 0; f < sl.nf8; ++f) split(dd_add(a0, dd_mul(D, (double)f)), sl.omr_hi[f], sl.omr_lo[f]);
    for (int b = 0; b < 8; ++b) split(dd_mul(D, (double)b), sl.step.hi[b], sl.step.lo[b]);
    return sl;
}
// Do the right-hand side's slots a + f*D ride the Gram's grid?  They are the modes s0/2 + f of the same step when s0 is even -> same
// grid, same coordinates.
inline bool rhs_on_grid(const ApSlots &sl) { return sl.s0 % 2 == 0 && sl.s0 / 2 + sl.nf8 <= sl.nsl; }
// ... mode (s0/2 + f) D is a + f D - delta/2: the residual joins the first-order term
inline std::vector<double> rhs_residuals(const ApSlots &sl) {
    std::vector<double> er(sl.eps.size());
    for (size_t f = 0; f < er.size(); ++f) er[f] = sl.eps[f] + 0.5 * sl.delta;
    return er;
}

// ---- slot sums by non-uniform FFT (nufft.hip): the limits -------------------------------------------------------------------------------
constexpr int kNufftMinGrid = 256;
constexpr double kNufftOversampling = 3.9;       // grid cells per slot: oversampling ~2 of the two-sided mode range
constexpr int kNufftMaxGrid = 8192;              // at least two grids of nf 64-bit cells have to fit the LDS
constexpr int64_t kNufftMinSamples = 4096;
constexpr int64_t kNufftMaxWeights = 256;        // weight vectors (activation pairs) of one call
constexpr int kNufftWindowsMaxGrid = 4096;       // batched windows: four grids of nf 64-bit cells in LDS
constexpr int64_t kNufftWindowsMinSamples = 2048, kNufftWindowsMinSlots = 64;

// fine grid for nslots modes: the smallest power of two >= 3.9 nslots, at least 256
inline int nufft_grid_size(int64_t nslots) {
    int nf = kNufftMinGrid;
    while ((double)nf < kNufftOversampling * (double)nslots) nf *= 2;
    return nf;
}
inline bool nufft_applicable(int64_t N, int64_t nslots, int64_t nq) {
    return nufft_grid_size(nslots) <= kNufftMaxGrid && N >= kNufftMinSamples && nq >= 1 && nq <= kNufftMaxWeights;
}
inline bool nufft_windows_applicable(int64_t n, int64_t nslots) {
    return n >= kNufftWindowsMinSamples && nslots >= kNufftWindowsMinSlots && nufft_grid_size(nslots) <= kNufftWindowsMaxGrid;
}

// ---- the dense forms (gram.hip): tiles, sample chunks, LDS images -----------------------------------------------------------------------
constexpr int kGramTileRows = 128, kGramTileCols = 256;   // a work item's output tile
constexpr int kGramChunkAlign = 64;                       // sample chunks are multiples of this (every stage depth divides it)
constexpr int64_t kGramMinStagesPerChunk = 8;             // >= 512 samples per chunk
constexpr int64_t kGramCUs = 256, kGramItemsPerCU = 16;   // the split aims at 16 work items per CU, in whole rounds of the 256 CUs
constexpr size_t kGramLdsBudget = 160 * 1024;
enum { kGramModeKr = 0, kGramModePanel = 1, kGramModeKrs = 2 };   // gram_kernel's MODE
constexpr int kGramPanelStage = 16;                       // the panel form has one instance: 2 x 48 KiB of LDS

struct GramTile { int i, j; };   // (ti, tj); gram.hip copies the lists to the device as int2
// lower-triangle 128x256 tiles of an n x n Gram
inline std::vector<GramTile> make_tiles(int64_t n) {
    std::vector<GramTile> tl;
    const int64_t nti = ceil_div(n, kGramTileRows);
    for (int64_t ti = 0; ti < nti; ++ti)
        for (int64_t tj = 0; tj <= ti / 2; ++tj) tl.push_back(GramTile{(int)ti, (int)tj});
    return tl;
}
// KRS tiles: rows p in [0,2Nf), columns q = p'*P + pair; tile needed when its first column's p' <= its last row
inline std::vector<GramTile> make_tiles_pairs(int64_t np2, int64_t P) {
    std::vector<GramTile> tl;
    const int64_t TM = kGramTileRows, TN = kGramTileCols, nti = ceil_div(np2, TM), ntj = ceil_div(np2 * P, TN);
    for (int64_t ti = 0; ti < nti; ++ti) {
        const int64_t plast = (ti * TM + TM - 1 < np2 - 1) ? ti * TM + TM - 1 : np2 - 1;
        for (int64_t tj = 0; tj < ntj; ++tj)
            if ((tj * TN) / P <= plast) tl.push_back(GramTile{(int)ti, (int)tj});
    }
    return tl;
}

struct GramPlan {
    int64_t n = 0;       // unknowns (valid columns)
    int64_t N = 0;       // samples
    int64_t tiles = 0;   // lower-triangle 128x256 tiles
    int64_t ksplit = 0;  // sample chunks
    int64_t rows_per_chunk = 0;
    size_t slab_bytes = 0;
    int64_t pairs = 0;   // KRS: nb(nb+1)/2, else 0
    int64_t np2 = 0;     // KRS: row space 2Nf
};
// split the samples so that (tiles x chunks [x problems of a batch]) fills the 256 CUs in whole rounds
inline void choose_split(GramPlan &pl, int64_t N, int64_t nbatch = 1) {
    const int64_t nstage = ceil_div(N, kGramChunkAlign);
    const int64_t max_split = nstage / kGramMinStagesPerChunk > 0 ? nstage / kGramMinStagesPerChunk : 1;
    int64_t want = ceil_div(kGramCUs * kGramItemsPerCU, pl.tiles * nbatch);
    if (want > max_split) want = max_split;
    int64_t best = 1; double best_eff = -1;
    for (int64_t ks = want / 2 > 0 ? want / 2 : 1; ks <= want * 2 && ks <= max_split; ++ks) {
        const int64_t items = pl.tiles * ks * nbatch;
        const double eff = (double)items / (double)(ceil_div(items, kGramCUs) * kGramCUs);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = ks; }
    }
    pl.ksplit = best;
    pl.rows_per_chunk = round_up(ceil_div(N, pl.ksplit), kGramChunkAlign);
    pl.slab_bytes = sizeof(double) * (size_t)pl.tiles * (size_t)pl.ksplit * kGramTileRows * kGramTileCols;
}
inline GramPlan make_gram_plan_pairs(int64_t Nf, int64_t nb, int64_t N) {
    GramPlan pl;
    pl.n = 2 * Nf * nb; pl.N = N; pl.pairs = nb * (nb + 1) / 2; pl.np2 = 2 * Nf;
    pl.tiles = (int64_t)make_tiles_pairs(pl.np2, pl.pairs).size();
    choose_split(pl, N);
    return pl;
}
inline GramPlan make_gram_plan(int64_t n, int64_t N, int64_t nbatch = 1) {   // nbatch: problems solved together
    GramPlan pl;
    pl.n = n; pl.N = N;
    pl.tiles = (int64_t)make_tiles(n).size();
    choose_split(pl, N, nbatch < 1 ? 1 : nbatch);
    return pl;
}

// LDS bytes of gram_kernel<mode, BK>: two stage images (upper bounds of what a tile stages), each part rounded up to whole 1 KiB DMA pieces
inline size_t gram_lds_bytes(int mode, int BK, int64_t nb, int64_t ldk) {
    const int TM = kGramTileRows, TN = kGramTileCols;
    int img, aux;
    if (mode == kGramModeKr) {
        const int g2 = (int)(2 * nb);
        const int nfI = (TM + g2 - 2) / g2 + 1, nfJ = (TN + g2 - 2) / g2 + 1;  // upper bounds
        img = BK * (nfI + nfJ) * 2;
        aux = (int)(BK * ldk);
    } else if (mode == kGramModeKrs) {
        const int P = (int)(nb * (nb + 1) / 2);
        const int nfI = TM / 2 + 1, nfJ = ((TN + P - 2) / P + 1) / 2 + 2;     // upper bounds
        img = BK * (nfI + nfJ) * 2;
        aux = (int)(BK * ldk);
    } else {
        img = BK * (TM + TN);
        aux = BK;
    }
    const int img_pad = (img + 127) & ~127, aux_pad = (aux + 127) & ~127;
    return sizeof(double) * 2 * (size_t)(img_pad + aux_pad);
}
// samples per stage of the instance a launcher takes: the deepest stage whose two LDS images fit (few basis functions -> many
// frequencies per tile), 0 when none does.  Instances exist at 32, 16, 8 (KR), 32, 16 (KRS; ldk = pairs) and 16 (PANEL: 2 x 48 KiB).
inline int gram_stage_for(int mode, int64_t nb, int64_t ldk) {
    const int deepest = mode == kGramModePanel ? kGramPanelStage : 32, shallowest = mode == kGramModeKr ? 8 : 16;
    for (int bk = deepest; bk >= shallowest; bk /= 2)
        if (gram_lds_bytes(mode, bk, nb, ldk) <= kGramLdsBudget) return bk;
    return 0;
}
// does the symmetric-pair form fit LDS for this many basis functions?  (one basis function has no pairs to save)
inline bool gram_krs_fits(int64_t nb) {
    const int64_t P = nb * (nb + 1) / 2;
    return nb >= 2 && gram_lds_bytes(kGramModeKrs, 16, nb, P) <= kGramLdsBudget;
}

// ---- the form decision --------------------------------------------------------------------------------------------------------------------
// LPVS_OPT_GRAM_FORM = auto (0, default) | LPVS_GRAM_AP | LPVS_GRAM_KRS | LPVS_GRAM_KR
//   ap : the grid is an arithmetic progression up to rounding (make_ap_slots admits it) -> 3Nf-1 non-uniform Fourier sums per
//        activation pair (nudft.hip), by non-uniform FFT (nufft.hip) when ONE progression serves all slots (merged layout), the
//        sizes are within its limits and LPVS_OPT_SLOT_SUMS does not say direct
//   krs / kr / panel : dense MFMA contraction for arbitrary grids (gram.hip); the LPV constructors take the symmetric-pair form
//        unless the option says kr or the pair table does not fit LDS, the Fourier constructor and the window engine the panel form
// The values are the codes lpvs_problem_get_timing reports as gram_form.  refused: LPVS_GRAM_AP was asked for and the grid is not
// admitted (the entry points answer LPVS_EARGUMENT).
enum class GramForm { refused = 0, kr = 1, krs = 2, panel = 3, ap = 4, ap_nufft = 5 };
enum class GramFamily { lpv, fourier, windows };   // whose Gram: the LPV constructors, lpvs_problem_create_fourier_f64, the window engine
inline bool gram_option_wants_slots(int option) { return option == 0 || option == LPVS_GRAM_AP; }   // else the grid is not even looked at
struct GramFormFacts {
    GramFamily family = GramFamily::lpv;
    int option = 0;                 // LPVS_OPT_GRAM_FORM in effect
    bool slots_ok = false, merged = false;   // of make_ap_slots (not called: false)
    bool slots_direct = false;      // LPVS_OPT_SLOT_SUMS in effect is LPVS_SLOTS_DIRECT
    int64_t N = 0;                  // samples (windows: of one window)
    int64_t nsl = 0;                // slots
    int64_t nq = 0;                 // lpv: activation pairs nb (nb + 1) / 2
    int64_t nb = 0;                 // lpv: basis functions
};
inline bool is_structured(GramForm f) { return f == GramForm::ap || f == GramForm::ap_nufft; }
inline GramForm choose_gram_form(const GramFormFacts &f) {
    const bool admitted = gram_option_wants_slots(f.option) && f.slots_ok;
    if (f.option == LPVS_GRAM_AP && !admitted) return GramForm::refused;
    if (admitted) {
        const bool in_limits = f.family == GramFamily::lpv ? nufft_applicable(f.N, f.nsl, f.nq)
                                                           : (f.family == GramFamily::windows && nufft_windows_applicable(f.N, f.nsl));
        return !f.slots_direct && f.merged && in_limits ? GramForm::ap_nufft : GramForm::ap;
    }
    if (f.family != GramFamily::lpv) return GramForm::panel;
    return f.option != LPVS_GRAM_KR && gram_krs_fits(f.nb) ? GramForm::krs : GramForm::kr;
}

// ---- what lpvs_problem_get_timing reports as work ----------------------------------------------------------------------------------------
inline double gram_flops(int64_t N, int64_t n) { return (double)N * (double)n * (double)(n + 1); }   // the lower triangle's algorithmic work
// flops the MFMA core issues: every tile whole, over the padded samples
inline double dense_issued_flops(const GramPlan &pl) { return (double)pl.tiles * 128.0 * 256.0 * 2.0 * (double)(pl.ksplit * pl.rows_per_chunk); }
// flops the structured form issues: 4 fma per sample, slot and weight vector (nq: activation pairs; Fourier: 1)
inline double structured_issued_flops(int64_t N, int64_t nsl, int64_t nq) { return 8.0 * (double)N * (double)nsl * (double)nq; }

}  // namespace lpvs
