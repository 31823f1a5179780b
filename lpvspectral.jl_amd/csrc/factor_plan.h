// factor_plan.h -- which launch schedule and which kernels a factorisation runs ("plan and schedules"): the knobs, parsed
// once, and the size thresholds, turned into a FactorPlan of choices.  linalg.hip launches what the plan says and decides nothing more.
// No HIP dependency: the host-side test (tests/test_factor_plan.py) compiles it as it is.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace lpvs {

// ---- thresholds on the padded size np ----------------------------------------------------------------------------------------------
constexpr int64_t kTwoLevelMinNp = 1024;    // below: the single-level 64-wide sweep
constexpr int64_t kGroupMinNp = 2048;       // from here the group schedule (one pass over A per group of 128-wide steps) replaces the steps
// depth-2 look-ahead of the steps schedule, measured at np = 8192: 18.4 -> 17.8 ms; neutral at 16384, slightly slower at 4096 (5.6 -> 5.8 ms)
constexpr int64_t kDepth2MinNp = 6144;
// band launches on 64 x 64 tiles (rank_updateb_kernel) below: 4.31 -> 3.98 ms at 4096; from 8192 the deep pass is the critical path either
// way (side chain 445 -> 390 us per pair against a 393-us deep pass; 12.9-13.1 ms with 128 x 128 band tiles, 13.1-13.3 with 64 x 64)
constexpr int64_t kBandTile128MinNp = 8192;
// From here the main pass is long enough to cover a four-step side chain: 84.5 ms with groups of four and 8-pivot stages against 89.6 with
// pairs at np = 16384 (tools/factor_ab4.sh); the pivot kernel alone on its CU waits too long for an empty one (84.5 -> 86.3 ms at 16384);
// and the steps schedule hides a 256-wide chain under its bulk update, which then runs closer to the MFMA peak.
constexpr int64_t kLargeNp = 12288;

// ---- the ten knobs, each string parsed here and nowhere else -------------------------------------------------------------------------
enum class PivotKnob { unset, regs, sweep64 };
enum class Lookahead { automatic, off, one };

struct FactorKnobs {
    bool factor_sweep64 = false;                // LPVS_FACTOR=sweep64: the single-level sweep at every size
    bool scheme_steps = false;                  // LPVS_FACTOR_SCHEME=steps: never the group schedule
    PivotKnob pivot = PivotKnob::unset;         // LPVS_PIVOT=regs|sweep64
    Lookahead lookahead = Lookahead::automatic; // LPVS_LOOKAHEAD: first character '0' off, '1' depth one
    int kw = 0;                                 // LPVS_KW=128|256: width of the outer pivot blocks
    bool chain_split = false;                   // LPVS_CHAIN=split: gather + GEMM instead of the fused panel kernel
    int group = 0;                              // LPVS_FACTOR_GROUP=1 .. 4: panels per pass (diagnostic)
    int ru_stage = 0;                           // LPVS_RU_STAGE=8|16: pivots per LDS stage of the deep pass
    int band_tile = 0;                          // LPVS_BAND_TILE=64|128
    int pivot_alone = -1;                       // LPVS_PIVOT_ALONE=0|1
};

// get: any callable  const char *(const char *name)  that answers nullptr for an unset knob (linalg.hip: experiment_env)
template <class Get>
FactorKnobs factor_knobs_from(Get get) {
    const auto is = [&](const char *name, const char *value) { const char *e = get(name); return e && strcmp(e, value) == 0; };
    const auto number = [&](const char *name, int unset) { const char *e = get(name); return e ? atoi(e) : unset; };
    FactorKnobs k;
    k.factor_sweep64 = is("LPVS_FACTOR", "sweep64");
    k.scheme_steps = is("LPVS_FACTOR_SCHEME", "steps");
    if (const char *e = get("LPVS_PIVOT")) k.pivot = strcmp(e, "regs") == 0 ? PivotKnob::regs : (strcmp(e, "sweep64") == 0 ? PivotKnob::sweep64 : PivotKnob::unset);
    if (const char *e = get("LPVS_LOOKAHEAD")) k.lookahead = e[0] == '0' ? Lookahead::off : (e[0] == '1' ? Lookahead::one : Lookahead::automatic);
    k.kw = number("LPVS_KW", 0);
    k.chain_split = is("LPVS_CHAIN", "split");
    k.group = number("LPVS_FACTOR_GROUP", 0);
    k.ru_stage = number("LPVS_RU_STAGE", 0);
    k.band_tile = number("LPVS_BAND_TILE", 0);
    k.pivot_alone = number("LPVS_PIVOT_ALONE", -1);
    return k;
}

// ---- the plan: choices only ----------------------------------------------------------------------------------------------------------
constexpr int kFactorGroupMax = 4;                                   // panels the deep pass takes at most (linalg.hip: kMaxGroup)
enum class FactorLevel { single, two };                              // single: sweep64 over the whole matrix
enum class FactorSchedule { groups, steps_depth2, steps_depth1, steps_serial };
enum class PivotKernel { mfma, regs, sweep64 };                      // pivot_inverse_mfma_kernel | pivot_inverse_kernel<128> | extract + 64-wide sweep

// A field that a schedule does not read holds the one value written beside it, so that two plans are equal exactly when they launch
// the same kinds of kernels in the same order.  The single-level sweep reads nothing: its plan is FactorPlan{}.
struct FactorPlan {
    FactorLevel level = FactorLevel::single;
    FactorSchedule schedule = FactorSchedule::steps_serial;
    int kw_outer = 128;                             // 128 | 256 (groups: 128)
    PivotKernel pivot = PivotKernel::sweep64;       // of a 128-wide pivot block; a 256-wide one is always extracted and swept
    bool fused_chain = false;                       // groups only (steps: gather + GEMM)
    int group_max = 1;                              // groups only: 1 .. 4 panels per pass
    int ru_stage = 16;                              // groups only: 8 | 16
    int band_tile = 128;                            // groups only: 64 | 128
    bool pivot_alone = false;                       // groups only: the pivot kernel asks for the rest of a CU's LDS (needs the CU-masked stream: linalg.hip)
};

// np: the padded size (a multiple of 128); have_aux: the caller brought side streams and events (SweepAux)
inline FactorPlan factor_plan(int64_t np, int nbatch, bool have_aux, const FactorKnobs &k) {
    FactorPlan p;
    if (!(nbatch == 1 && np >= kTwoLevelMinNp && !k.factor_sweep64)) return p;
    p.level = FactorLevel::two;
    // 128-wide pivot blocks (one-workgroup inverse); the steps schedule takes 256-wide ones from kLargeNp (the group schedule runs 128-wide
    // steps: 39.9 ms against 47.5 with 256-wide steps at np = 12288, 89.5 / 93.5 at 16384, equal at 32768)
    p.kw_outer = k.kw == 128 || k.kw == 256 ? k.kw : ((k.scheme_steps && np >= kLargeNp) ? 256 : 128);
    const bool la = k.lookahead != Lookahead::off && have_aux && np > p.kw_outer;
    if (la && !k.scheme_steps && k.pivot != PivotKnob::sweep64 && p.kw_outer == 128 && np >= kGroupMinNp) {
        p.schedule = FactorSchedule::groups;
        p.pivot = k.pivot == PivotKnob::regs ? PivotKernel::regs : PivotKernel::mfma;
        p.fused_chain = !k.chain_split;
        // Measured at np = 8192 (tools/factor_ab3.sh): 1 panel per pass 16.2 ms, 2: 14.0, 3: 15.0, 4: 15.4 (from mg = 3 the side stream is
        // the critical path again: linalg.hip)
        p.group_max = k.group >= 1 && k.group <= kFactorGroupMax ? k.group : (np >= kLargeNp ? 4 : 2);
        // 8-pivot LDS stages (32 KB per workgroup) and a register budget for three workgroups per CU: np = 8192: 14.65 ms against 13.3 with
        // 16-pivot stages and two workgroups per CU; np = 16384: 84.5 against 86.5
        p.ru_stage = k.ru_stage == 8 || (k.ru_stage != 16 && np >= kLargeNp) ? 8 : 16;
        p.band_tile = k.band_tile == 64 || (k.band_tile != 128 && np < kBandTile128MinNp) ? 64 : 128;
        p.pivot_alone = k.pivot_alone >= 0 ? k.pivot_alone != 0 : np < kLargeNp;     // np = 8192: 13.5 -> 13.2 ms
        return p;
    }
    p.schedule = !la ? FactorSchedule::steps_serial
                     : (np >= kDepth2MinNp && k.lookahead != Lookahead::one ? FactorSchedule::steps_depth2 : FactorSchedule::steps_depth1);
    // (with 256-wide blocks only a ragged last block is 128 wide: without one the field keeps its fixed value)
    const bool has_128_block = p.kw_outer == 128 || np % 256 != 0;
    if (has_128_block && k.pivot != PivotKnob::sweep64) p.pivot = PivotKernel::regs;
    return p;
}

}  // namespace lpvs
