// eval_plan.h -- the host-side decisions of model evaluation (predict / residual / fva: eval.hip): whether a frequency
// grid is admitted to the type-2 non-uniform FFT and with which fine grid, which path `auto` takes, how the direct path tiles its
// accumulators over basis functions and coefficient columns, and how many partial sums the residual epilogue leaves.
// Pure functions of numbers: api.hip and eval.hip allocate and launch what they say and compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_eval_plan.py) compiles it as it is.
#pragma once

#include "gram_form_plan.h"

namespace lpvs {

// ---- admission -----------------------------------------------------------------------------------------------------------------------------
// w_f = a + f D + eps_f is evaluated as  e^{i a x} sum_f p_f (1 + i eps_f x) e^{i f D x}:  modes 0 .. Nf-1 of ONE step D on a fine grid of
// nufft_grid_size(Nf) points.  The residual rule is make_ap_slots' (max|eps| max|x| <= kApMaxResidualPhase: the dropped second-order
// term is <= 5e-15); the grid is held to kNufftMaxGrid.  A grid of one frequency or of step 0 has no progression to speak of.
struct EvalGrid {
    bool progression = false;   // make_ap_slots admits the grid (and it has a step)
    bool ok = false;            // ... and the fine grid is within kNufftMaxGrid: the type-2 path may run
    bool twin = false;          // some eps_f != 0: the first-order twin grids run
    int nf = 0;                 // fine grid (0: beyond the limit or no progression)
    double emax = 0;            // max|eps_f|
    double a = 0;               // first frequency (exact: it is w[0])
    double D_hi = 0, D_lo = 0;  // the step in double-double
    std::vector<double> eps;
};
inline EvalGrid eval_admit(const std::vector<double> &hw, double xam) {
    EvalGrid g;
    if (hw.size() < 2) return g;
    const ApSlots sl = make_ap_slots(hw, xam, false);
    g.emax = sl.emax;
    g.eps = sl.eps;
    if (!sl.ok || !(sl.step.hi[1] != 0.0) || !std::isfinite(sl.step.hi[1])) return g;
    g.progression = true;
    g.a = hw[0]; g.D_hi = sl.step.hi[1]; g.D_lo = sl.step.lo[1];
    for (double e : g.eps) g.twin = g.twin || e != 0.0;
    const int nf = nufft_grid_size((int64_t)hw.size());
    if (nf > kNufftMaxGrid) return g;
    g.nf = nf; g.ok = true;
    return g;
}

// ---- the path ------------------------------------------------------------------------------------------------------------------------------
enum { kEvalPathAuto = 0, kEvalPathDirect = 1, kEvalPathNufft = 2, kEvalPathRefused = -1 };
// `auto` takes the type-2 path from this many samples on.  The grids cost O(nf Nf) per basis function and column whatever M is, the
// interpolation 16 grid values per sample against Nf sincos of the direct path.  Measured (profiles/predict_time.txt): at Nf = 512 the type-2
// path is ahead at every M from 2^10 (0.19 against 0.35 ms of device time), at Nf = 32 the direct path stays 0.03 ms ahead up to 2^18: the
// crossover moves with Nf, both differences are of the size of a launch, and the structured Gram's threshold sits between them.
constexpr int64_t kEvalNufftMinSamples = kNufftMinSamples;
inline int eval_choose_path(int requested, bool grid_ok, int64_t M) {
    if (requested == kEvalPathDirect) return kEvalPathDirect;
    if (requested == kEvalPathNufft) return grid_ok ? kEvalPathNufft : kEvalPathRefused;
    if (requested != kEvalPathAuto) return kEvalPathRefused;
    return grid_ok && M >= kEvalNufftMinSamples ? kEvalPathNufft : kEvalPathDirect;
}

// ---- the direct path's accumulators --------------------------------------------------------------------------------------------------------
// A thread owns one sample and kEvalBasisTile x tc accumulators (basis functions x coefficient columns, tc in {1, 4, 8}: at most 64
// doubles, which stay in registers); more basis functions are further passes over the frequencies in the same thread, more columns are
// further workgroups (blockIdx.y).  One sincos per (sample, frequency) and pass.
constexpr int kEvalBlock = 256;          // samples per workgroup, both paths
constexpr int kEvalBasisTile = 8;
constexpr int kEvalFreqChunk = 32;       // frequencies whose coefficients are staged in LDS at a time: 32 x 8 x 8 x 16 B = 32 KiB at most
struct EvalTiling { int tj = 0, tc = 0, jpasses = 0, cblocks = 0, acc = 0; };
inline EvalTiling eval_tiling(int64_t nb, int64_t nc) {
    EvalTiling t;
    t.tj = (int)(nb < kEvalBasisTile ? nb : kEvalBasisTile);
    t.tc = nc <= 1 ? 1 : (nc <= 4 ? 4 : 8);
    t.jpasses = (int)ceil_div(nb, kEvalBasisTile);
    t.cblocks = (int)ceil_div(nc, t.tc);
    t.acc = kEvalBasisTile * t.tc;
    return t;
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------------------
// every workgroup leaves one partial of sum(e) and sum(e^2) per column (a pairwise tree over its 256 samples); one workgroup per column then
// adds the slabs: thread t the slabs t, t + 256, ... in ascending order, then a pairwise tree over the 256 threads
inline int64_t eval_sum_slabs(int64_t M) { return ceil_div(M, kEvalBlock); }

}  // namespace lpvs
