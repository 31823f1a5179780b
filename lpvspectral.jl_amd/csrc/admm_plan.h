// admm_plan.h -- the host-side decisions of the ADMM handle (api.hip): after which iterations the x-update is corrected,
// how the packed inverse is stored and read, which iteration a handle or a batch runs, and how a run is cut into graph replays and
// sub-chunks.  Pure functions of numbers, flags and strings: api.hip and the admm*.hip units allocate and launch what they say and
// compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_admm_plan.py) compiles it as it is.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/lpvspectral.h"
#include "windows_plan.h"

namespace lpvs {

constexpr int64_t kSymmetricMinNp = 2048;  // below this the iteration is launch-latency bound: plain mat-vec on the full matrix, no packed copy

// ---- the correction schedule (admm_refine.hip, launch_xupdate_correction) -----------------------------------------------
// Default: every handle of n >= 2048.  Round 6: handles with several right-hand sides too -- at cfg5's judged size (n = 32768, 8 channels)
// the uncorrected run drifts 4.1e-10 in x, z (1.4e-10 in u) from the corrected one after 2000 iterations
// (profiles/r06_cfg5_xcorr_fullsize.txt), the same constant forcing E w as at cfg3; a correction there is an accurate product over the
// 8.6-GB f64 Gram for all channels in one pass: 8.6 ms, three of them 1.9 % of a 2000-iteration run.  LPVS_XCORR_OFF switches it off per handle.
// Schedule (round 6): after 16, then 128 and its doublings for one right-hand side (five corrections in 2000 iterations: +0.4 ms at cfg3) --
// the off-family sweep (tests/test_gpu_offfamily.py, profiles/r06_offfamily_probe*.txt) has cases at cond(G + I/mu) ~ 2e4 where 16, 512, ...
// leaves x, z 8e-10 from the exact iterates after 600 iterations and this schedule 1.5e-10; 512 and its doublings for several right-hand
// sides (a correction there is a pass over the whole f64 Gram for all channels: 8.6 ms at cfg5; measured 2.6e-10 from the CPU reference
// iterates at n = 8192: tests/test_gpu_configs.py).
constexpr int kXcorrFirst = 16;              // the one correction before the schedule's own first point
constexpr int kXcorrEveryOneRhs = 128;       // then after this iteration and its doublings: one right-hand side
constexpr int kXcorrEverySeveralRhs = 512;   // ... several

// after the iterations base^j (base >= 2), or after iteration 16 and every `every`-th one (doubling: every, 2 every, 4 every, ...);
// base = every = 0: no correction
struct XcorrSchedule {
    int base = 0, every = 0;
    bool doubling = false, early = false;
    bool on() const { return base >= 2 || every > 0; }
    // the first scheduled iteration after k.  An absolute function of k: the iterates do not depend on the chunking.
    long long next(long long k) const {
        if (every > 0 && doubling) {   // 16 (early: 1, 2, 4, 8, 16), then `every` and its doublings: the iterates move ever more slowly
            if (early && k < kXcorrFirst) { long long q = 1; while (q <= k) q *= 2; return q; }
            if (k < kXcorrFirst && every > kXcorrFirst) return kXcorrFirst;
            long long q = every;
            while (q <= k) q *= 2;
            return q;
        }
        if (every > 0) { if (k < kXcorrFirst && every > kXcorrFirst) return kXcorrFirst; return (k / every + 1) * (long long)every; }
        long long q = 1;
        while (q <= k) q *= base;
        return q;
    }
};
inline XcorrSchedule xcorr_default_schedule(int64_t ns, bool corrected) {
    XcorrSchedule s;
    s.every = corrected ? (ns == 1 ? kXcorrEveryOneRhs : kXcorrEverySeveralRhs) : 0;
    s.doubling = true;
    return s;
}
// LPVS_XUPDATE_CORRECTION as a schedule experiment (A/B measurements): "B" after B^j; "eN" after 16 and every N-th; "dN" after 16, N, 2N,
// 4N, ...; "qN" after 1, 2, 4, 8, 16, N, 2N, 4N, ...  "0" only says off, and only as the option's last fallback (option_from_env), not here.
// Anything else ("1", "on", "true", "e0", ...) only says ON: the default schedule stays ("1" used to fall through to
// base = 0, i.e. silently OFF, and took the 32-bit reads with it).
inline XcorrSchedule xcorr_schedule_from(const char *e, XcorrSchedule dflt) {
    if (e == nullptr || (e[0] == '0' && e[1] == 0)) return dflt;
    XcorrSchedule s = dflt;
    if ((e[0] == 'e' || e[0] == 'd' || e[0] == 'q') && atoi(e + 1) > 0) {
        s.base = 0; s.every = atoi(e + 1);
        s.doubling = e[0] == 'd' || e[0] == 'q'; s.early = e[0] == 'q';
    } else if (e[0] >= '0' && e[0] <= '9' && atoi(e) >= 2) { s.every = 0; s.base = atoi(e); }
    return s;
}

// ---- the storage of the packed inverse ------------------------------------------------------------------------------------------------
// LPVS_M_STORAGE = mixed (default) | split | f64: how a double-precision handle stores the tile-packed inverse its mat-vec streams.
// split = float head + 16-bit tail (6 bytes, 40 significant bits, admm.hip); mixed = the same, except that
// tiles whose entries are all small against max|M| (the off-diagonal tiles of the LPV / Fourier inverses) are 36-bit fixed point
// (4.53 bytes per element); _f32 handles always stream floats.  Handles with several right-hand sides decode either format on
// the way into the LDS image their matrix-core tile product reads (their diagonal tiles always stay 6-byte).
enum { kMpNone = 0, kMpF64 = 1, kMpF32 = 2, kMpSplit = 3, kMpMixed = 4 };
constexpr int64_t kSeveralRhsPackedMaxNp = 49152;   // the streaming multi-signal kernel addresses its partials with 31-bit byte offsets
constexpr int kFixBitsAll = 36, kFixBitsLeast = 20;  // significant bits of a fixed-point tile (32: nibbles zero and not read)

inline size_t storage_element_bytes(int mode) { return mode == kMpF32 ? 4 : (mode == kMpSplit || mode == kMpMixed ? 6 : (mode == kMpF64 ? 8 : 0)); }

// multi_fixed_ok: the multi-signal tile product in use reads fixed-point off-diagonal tiles (admm_multi.hip: multi_signal_fixed_tiles_ok)
inline int storage_mode(int64_t np, int64_t ns, bool f32, int storage_option, bool multi_fixed_ok) {
    if (np < kSymmetricMinNp) return kMpNone;
    if (f32) return kMpF32;
    if (storage_option == LPVS_STORAGE_F64) return kMpF64;
    if (ns > 1 && np > kSeveralRhsPackedMaxNp) return kMpF64;
    if (storage_option == LPVS_STORAGE_SPLIT) return kMpSplit;
    if (ns > 1 && !multi_fixed_ok) return kMpSplit;
    return kMpMixed;   // (several right-hand sides: diagonal tiles always float-head)
}

// LPVS_NIB_PERIOD, LPVS_NIB_RAMP (experiments): refresh period of the stale nibble product (0: none, the 36-bit reads) and the ramp that
// makes it denser while the right-hand side still moves fast -- after every launch up to 15, every 2nd up to 31, 4th up to 63, ..., 32nd
// from 256 on (103 refreshes in 2000 iterations; u at cfg3 after 200 iterations 1.75e-10 from the exact iterate instead of 3.9e-10 --
// 36-bit reads: 1.40e-10)
struct NibKnobs { int period = 32, ramp = 8; };
// get: any callable  const char *(const char *name)  that answers nullptr for an unset knob (api.hip: experiment_env)
template <class Get>
NibKnobs nib_knobs_from(Get get) {
    NibKnobs k;
    if (const char *e = get("LPVS_NIB_PERIOD")) k.period = atoi(e) > 0 ? atoi(e) : 0;
    if (const char *e = get("LPVS_NIB_RAMP")) k.ramp = atoi(e) > 0 ? atoi(e) : 0;
    return k;
}
// LPVS_FIX_BITS (experiment): 20 .. 36, anything else leaves all 36 (the nibble planes feed the stale nibble product)
template <class Get>
int fix_bits_from(Get get) {
    const char *e = get("LPVS_FIX_BITS");
    return e && atoi(e) >= kFixBitsLeast && atoi(e) <= kFixBitsAll ? atoi(e) : kFixBitsAll;
}

// Corrected single-signal handles READ 32 bits of the 36 their fixed-point tiles hold (4 B per element instead of 4.5) and carry the
// product of the 4-bit planes with a right-hand side up to nib_period iterations old in the offset vector (admm.hip, "the stale nibble
// product"): x, z and u all stay where the 36-bit reads leave them (u within 5.0e-10 of the exact iterates at cfg3; plain truncation to
// 32 bits: 2e-9 .. 7e-9 -- the dual variable integrates it; profiles/r05_cfg3_stale_nibble_product.txt, r05_cfg3_fixbits.txt).
// The default, and LPVS_STORAGE_MIXED32 by name; LPVS_STORAGE_MIXED asks for the 36-bit reads.  (The window engine's one-launch batches
// follow the same rule: corrected = the batch iterates in one launch.)
inline bool storage_reads_32_bits(int64_t ns, bool f32, bool corrected, int storage_option) {
    return ns == 1 && !f32 && corrected && (storage_option == 0 || storage_option == LPVS_STORAGE_MIXED32);
}

struct StoragePlan {
    int mode = kMpNone;
    bool read32 = false;
    int fix_bits = kFixBitsAll;          // the fixed-point tiles are packed with this many significant bits
    int nib_period = 0, nib_ramp = 0;    // the stale nibble product's refreshes (0: none)
    size_t element_bytes = 0;
    size_t bytes = 0;                    // of the buffer: the elements; mixed: + tile formats + max|M| (packed_layout)
    bool diag_float = false;             // mixed, several right-hand sides: diagonal tiles always in the float-head format
    bool want_rowsum = false;            // mixed, one right-hand side: the packing pass also leaves the largest absolute row sum of M
    // reduced-precision copies of M (split, f32) are only ever applied to (z-u)/mu: x = xb + M~ (z-u)/mu, xb = M b in full precision
    // (round 5: the 8-byte storage too -- the offset vector is refined against a double-double residual, which the in-loop product
    // M (b + v) cannot be)
    bool offset_form = false;
    bool owns_fi = false;                // the handle holds records of the one-launch iteration (fi_doubles(np) doubles)
};
// storage_option: LPVS_OPT_M_STORAGE in effect; corrected: the handle's correction schedule is on
inline StoragePlan admm_storage_plan(int64_t np, int64_t ns, bool f32, int storage_option, bool multi_fixed_ok, bool corrected, int fix_bits_knob,
                                     NibKnobs nib) {
    StoragePlan p;
    p.mode = storage_mode(np, ns, f32, storage_option, multi_fixed_ok);
    // (on a handle the rule implies the mixed storage: one right-hand side, not f32, option 0 or MIXED32, corrected and so np >= kSymmetricMinNp)
    p.read32 = p.mode == kMpMixed && storage_reads_32_bits(ns, f32, corrected, storage_option);
    p.fix_bits = fix_bits_knob;
    p.nib_period = p.read32 ? nib.period : 0;
    p.nib_ramp = p.read32 ? nib.ramp : 0;
    p.element_bytes = storage_element_bytes(p.mode);
    if (p.mode != kMpNone) {
        const PackedLayout lay = packed_layout(np, p.element_bytes, 1);
        p.bytes = p.mode == kMpMixed ? lay.bytes : lay.elems_bytes;
    }
    p.diag_float = p.mode == kMpMixed && ns > 1;
    p.want_rowsum = p.mode == kMpMixed && ns == 1;
    p.offset_form = np >= kSymmetricMinNp;
    p.owns_fi = p.offset_form && ns == 1 && (p.mode == kMpMixed || p.mode == kMpF32);
    return p;
}
// Not a diagonally dominant inverse (fewer than half of the tiles qualified for fixed point): the mixed kernel (three workgroups per CU,
// float-head tiles in two halves) would only lose against the plain 6-byte kernel -- every tile is stored in the float-head format
inline bool demote_to_split(size_t fixed, size_t tiles) { return 2 * fixed < tiles; }
// ... and the plan of a handle whose mixed storage was demoted: split in the same buffer, no tile formats, so no 32-bit reads and no
// one-launch iteration
inline StoragePlan demoted_plan(StoragePlan p) {
    p.mode = kMpSplit; p.nib_period = 0; p.diag_float = p.want_rowsum = p.owns_fi = false;
    return p;
}
// Is the packed copy written again?  valid: it is the packed copy of the current M.  The same M packed with other fix bits does not
// count; a split copy that a demotion left counts as the mixed one asked for (mixed was tried for this M and found no small tiles).
inline bool must_repack(bool valid, int have_mode, int have_fix_bits, bool have_demoted, int want_mode, int want_fix_bits) {
    if (valid && have_mode == kMpMixed && have_fix_bits != want_fix_bits) valid = false;
    const bool demoted = want_mode == kMpMixed && have_mode == kMpSplit && have_demoted;
    return !valid || (have_mode != want_mode && !demoted);
}

// ---- which iteration runs ---------------------------------------------------------------------------------------------------------------
constexpr int64_t kOneLaunchMaxNp = 49152;        // six clamped loads per lane cover the block norms / maxima of 384 row blocks; the quantum bound of admm_one_launch.hip
constexpr int kSmallMaxNp = 2048;                 // admm_small.hip: LDS image of the right-hand side (np < kSymmetricMinNp anyway)
constexpr int64_t kSmallMinNp = 128;
constexpr int64_t kSmallMaxGroupLen = 256;
constexpr int64_t kBatchOneLaunchMaxNp = 8192;    // up to 64 row blocks: one clamped load per lane
constexpr int64_t kBatchMaxStateBytes = (int64_t)1 << 40;

struct IterFacts {
    int64_t np = 0, n = 0;
    int ns = 1;                       // right-hand sides of a handle
    int prox_kind = LPVS_PROX_L1;
    int64_t group_len = 0;
    bool option_two = false;          // LPVS_OPT_ITERATION in effect is LPVS_ITERATION_TWO
    bool packed = false, partials = false, offset = false, tile_formats = false, split_copy = false, f32_copy = false;   // what the parameters hold
    bool fi = false, small_ctl = false, scratch = false;
    int nrhs = 1;                     // batch: problems per matrix
    int64_t nbatch = 0;               // batch: problems (0: a handle)
};
enum class IterationKind { two_launch, one_launch, small_one_launch, batch_one_launch };

// can the update ride the tile partials' consumers?  (IndBallL0 needs the whole vector; a group must not straddle two row blocks)
inline bool prox_fusable(const IterFacts &f) {
    if (f.prox_kind == LPVS_PROX_L1 || f.prox_kind == LPVS_PROX_L0) return true;
    return f.prox_kind == LPVS_PROX_GROUP_L2 && f.group_len >= 1 && f.group_len <= kTile && kTile % f.group_len == 0 && f.n % f.group_len == 0;
}
inline bool one_launch_applies(const IterFacts &f) {
    return !f.option_two && f.fi && f.ns == 1 && (f.tile_formats || f.f32_copy) && f.offset && f.partials && f.packed && prox_fusable(f) &&
           f.np <= kOneLaunchMaxNp;
}
inline bool small_one_launch_applies(const IterFacts &f) {
    if (f.option_two || !f.small_ctl || f.packed || !f.scratch || f.np > kSmallMaxNp || f.np < kSmallMinNp || f.offset) return false;
    if (f.prox_kind == LPVS_PROX_L1 || f.prox_kind == LPVS_PROX_L0) return true;
    return f.prox_kind == LPVS_PROX_GROUP_L2 && f.group_len >= 1 && f.group_len <= kSmallMaxGroupLen && f.n % f.group_len == 0;
}
inline bool batch_one_launch_applies(const IterFacts &f) {
    return !f.option_two && f.fi && f.nrhs <= 1 && f.split_copy && f.tile_formats && f.offset && f.partials && f.packed && prox_fusable(f) &&
           f.np <= kBatchOneLaunchMaxNp && f.nbatch * f.np * 8 < kBatchMaxStateBytes;
}
inline IterationKind iteration_kind(const IterFacts &f) {
    if (f.nbatch > 0) return batch_one_launch_applies(f) ? IterationKind::batch_one_launch : IterationKind::two_launch;
    if (one_launch_applies(f)) return IterationKind::one_launch;
    return small_one_launch_applies(f) ? IterationKind::small_one_launch : IterationKind::two_launch;
}

// ---- how a run is cut -------------------------------------------------------------------------------------------------------------------
// np < kSymmetricMinNp: launches of a few microseconds each, host launch cost dominates, so a captured chunk is replayed while at least
// two chunks remain.  (The one-launch iteration of small problems pays two extra launches per chunk: longer chunks.)
constexpr int64_t kGraphItersSmallOneLaunch = 250, kGraphItersTwoLaunch = 50;
constexpr int64_t kGraphMinChunks = 2;
inline int64_t graph_chunk_iters(IterationKind kind) { return kind == IterationKind::small_one_launch ? kGraphItersSmallOneLaunch : kGraphItersTwoLaunch; }
inline int64_t graph_replays(int64_t np, int64_t todo, int64_t chunk, bool graphs_allowed) {
    return graphs_allowed && np < kSymmetricMinNp && todo >= kGraphMinChunks * chunk ? todo / chunk : 0;
}
// The correction schedule cuts the run at its iterations, whatever chunks the caller asks for: `step` iterations next (k_enqueued: since
// lpvs_admm_init / lpvs_admm_set_state; todo > 0: left of this call), then a correction or not.
struct RunStep { int64_t step = 0; bool correct_after = false; };
inline RunStep next_run_step(const XcorrSchedule &schedule, long long k_enqueued, int64_t todo) {
    RunStep r;
    r.step = todo;
    if (!schedule.on()) return r;
    const long long next = schedule.next(k_enqueued);
    if (next - k_enqueued < r.step) r.step = next - k_enqueued;
    r.correct_after = k_enqueued + r.step == next;
    return r;
}

// The stale nibble product is refreshed after the launches g that are multiples of the step of g's octave: 2^floor(log2 g) / ramp, between
// 1 and the period (g = 0 counts to the octave of 1); without a ramp after g = 1 and the multiples of the period.
inline long long nib_step(long long p2, int period, int ramp) {
    const long long step = p2 / ramp;
    return step < 1 ? 1 : (step > period ? period : step);
}
// is it refreshed after launch g?  An absolute function of g: the iterates do not depend on the chunking.
inline bool nib_refresh_due(long long g, int period, int ramp) {
    if (period <= 0) return false;
    if (ramp <= 0) return g == 1 || g % period == 0;
    long long p2 = 1;
    while (2 * p2 <= g) p2 *= 2;                      // 2^floor(log2 g)   (g = 0: 1)
    return g % nib_step(p2, period, ramp) == 0;
}
// refreshes due after the launches g0 <= g < g1: octave by octave, the multiples of one step each
inline long long nib_refreshes_between(long long g0, long long g1, int period, int ramp) {
    if (period <= 0 || g1 <= g0) return 0;
    const auto multiples = [](long long a, long long b, long long s) { return (b + s - 1) / s - (a + s - 1) / s; };   // of s in [a, b), 0 <= a <= b
    if (ramp <= 0) return multiples(g0, g1, period) + (period > 1 && g0 <= 1 && 1 < g1 ? 1 : 0);
    long long count = 0;
    for (long long p2 = 1; (p2 == 1 ? 0 : p2) < g1; p2 *= 2) {
        const long long lo = p2 == 1 ? 0 : p2, step = nib_step(p2, period, ramp);
        const long long a = g0 > lo ? g0 : lo;
        if (step == period) return count + multiples(a, g1, step);   // every later octave has the period's step
        const long long b = g1 < 2 * p2 ? g1 : 2 * p2;
        if (a < b) count += multiples(a, b, step);
    }
    return count;
}

}  // namespace lpvs
