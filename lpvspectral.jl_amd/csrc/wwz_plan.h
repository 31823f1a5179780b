// wwz_plan.h -- the host-side decisions of the weighted wavelet Z-transform (wwz: wwz.hip, api.hip; include/lpvspectral.h g8; DESIGN.md
// 4.16): the checks of the host arguments, the decay per frequency, the sort of the times into groups of TT adjacent values, how many times
// and signals a thread of the sums kernel carries, the tiles of frequencies, the samples a (group, tile) stages, their cut into slabs, the
// work list, the bytes of partial sums and the count of staged against useful (sample, frequency, time) triples.
// Pure functions of numbers: api.hip and wwz.hip allocate and launch what they say and compute none of this themselves.
// No HIP dependency: the host-side test (tests/test_wwz_plan.py) compiles it as it is.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "lomb_plan.h"

namespace lpvs {

enum { kWwzOk = 0, kWwzArgument = 1, kWwzUnsupported = 2 };

// ---- the weight ----------------------------------------------------------------------------------------------------------------------------
// g = exp(-a_k d^2), d = t - tau, with a_k = c (2 pi f_k)^2 formed ONCE per frequency in double as  w = 6.283185307179586 * f_k,
// a_k = c * (w * w)  (three roundings; the reference of the tests forms the same double)
inline double wwz_decay(double c, double f) {
    const double w = 6.283185307179586 * f;
    return c * (w * w);
}

// ---- times and signals per thread ----------------------------------------------------------------------------------------------------------
// A thread of the sums kernel serves one frequency, TT times and ts signals from ONE sincospi per sample: 6 sums per time that no signal
// enters (sum Wg, sum (Wg)^2, C, S, C2, S2) and 4 per time and signal (Y, YY, YC, YS), under the family's cap of 48 accumulators:
//   one signal:  ts = 1, TT = 4: 4 (6 + 4) = 40;     several: ts = 4 (blocks of four, as lomb_tiling), TT = 2: 2 (6 + 16) = 44.
// TT is then halved while half of it still holds the whole list (one time: 1; two: 2; three: 4, the last group padded).
constexpr int kWwzMaxAcc = 48, kWwzSharedSums = 6, kWwzSignalSums = 4;
inline void wwz_threads(int64_t ns, int64_t Ntau, int *TT, int *ts) {
    *ts = ns <= 1 ? 1 : 4;
    int tt = 4;
    while (tt > 1 && tt * (kWwzSharedSums + kWwzSignalSums * *ts) > kWwzMaxAcc) tt >>= 1;
    while (tt > 1 && tt / 2 >= Ntau) tt >>= 1;
    *TT = tt;
}

// ---- slabs ---------------------------------------------------------------------------------------------------------------------------------
// Slabs lie at ABSOLUTE multiples of a slab length that depends on N alone: at least kWwzMinSlab samples, and so long that the record holds
// at most kWwzSlabsPerRecord of them (a multiple of kLombStage).  A cell's sums are added per slab it touches and then in lomb_pairwise's
// tree over those slabs, counted from the cell's own first slab: the order depends on the cell's (start, count) and on N, on nothing else.
constexpr int64_t kWwzMinSlab = 1024, kWwzSlabsPerRecord = 64, kWwzMaxAxis = (int64_t)1 << 24;
static_assert(kWwzMinSlab % kLombStage == 0 && kWwzSlabsPerRecord + 1 <= kLombMaxSlabs, "no cell has more slabs than lomb_pairwise adds");
inline int64_t wwz_slab(int64_t N) {
    const int64_t L = round_up(ceil_div(N, kWwzSlabsPerRecord), kLombStage);
    return L < kWwzMinSlab ? kWwzMinSlab : L;
}

// ---- the shape of a call: everything that is known before the device has looked at t ------------------------------------------------------
struct WwzShape {
    int status = kWwzArgument;
    std::string why;                    // (refused: the reason)
    int TT = 0, ts = 0, acc = 0, sblocks = 0;
    int64_t ngroups = 0, ftiles = 0, slab_samples = 0, rows = 0;   // rows of partial sums per (item, time of the group): 6 + 4 ns
    std::vector<double> decay;          // [Nf]: a_k
    std::vector<int32_t> order;         // [Ntau]: order[p] = the caller's index of the p-th smallest time (ties: the caller's order)
    std::vector<int32_t> pos;           // [Ntau]: pos[j] = the place of the caller's time j; its group is pos / TT, its slot pos % TT
    std::vector<double> tau_sorted;     // [ngroups TT]: the last group is padded with the largest time (computed, never read)
    std::vector<double> gmin, gmax;     // [ngroups]: the first and last time of a group
    std::vector<double> rmax;           // [ftiles]: the largest radius of a tile (its lowest frequency, for radii that fall with f)
};
inline WwzShape wwz_shape(int64_t N, int64_t ns, const double *f, int64_t Nf, const double *tau, int64_t Ntau, double c, const double *radius) {
    WwzShape p;
    auto refuse = [&p](int status, const std::string &why) { p.status = status; p.why = why; return p; };
    auto ll = [](int64_t v) { return std::to_string((long long)v); };
    if (N < 1 || Nf < 1 || Ntau < 1 || ns < 1 || ns > 65535)
        return refuse(kWwzArgument, "wwz: need N > 0, Nf > 0, Ntau > 0 and 1 <= ns <= 65535 (N = " + ll(N) + ", Nf = " + ll(Nf) + ", Ntau = " + ll(Ntau) + ", ns = " + ll(ns) + ")");
    if (Nf > kWwzMaxAxis) return refuse(kWwzUnsupported, "wwz: " + ll(Nf) + " frequencies are more than 2^24");
    if (Ntau > kWwzMaxAxis) return refuse(kWwzUnsupported, "wwz: " + ll(Ntau) + " times are more than 2^24");
    if (!(c > 0.0) || !std::isfinite(c)) return refuse(kWwzArgument, "wwz: the decay c must be positive and finite");
    for (int64_t k = 0; k < Nf; ++k) {
        if (!std::isfinite(f[k])) return refuse(kWwzArgument, "wwz: a frequency is not finite");
        if (!(f[k] > 0.0)) return refuse(kWwzArgument, "wwz: frequency " + ll(k) + " is not positive");
        if (!(radius[k] > 0.0)) return refuse(kWwzArgument, "wwz: radius " + ll(k) + " is not positive (or not a number)");
    }
    for (int64_t j = 0; j < Ntau; ++j)
        if (!std::isfinite(tau[j])) return refuse(kWwzArgument, "wwz: a time tau is not finite");
    // a thread per (frequency, time, signal) in grids of 256, and per edge of a cell
    const double most = 255.0 * (double)kLombMaxGrid, cells = (double)Nf * (double)Ntau;
    if (cells * (double)ns > most || 2.0 * cells > most)
        return refuse(kWwzUnsupported, "wwz: " + ll(Nf) + " frequencies, " + ll(Ntau) + " times and " + ll(ns) + " signals are more than one call takes");
    wwz_threads(ns, Ntau, &p.TT, &p.ts);
    p.acc = p.TT * (kWwzSharedSums + kWwzSignalSums * p.ts);
    p.sblocks = (int)ceil_div(ns, p.ts);
    p.ngroups = ceil_div(Ntau, p.TT);
    p.ftiles = ceil_div(Nf, kLombFreqTile);
    p.slab_samples = wwz_slab(N);
    p.rows = kWwzSharedSums + kWwzSignalSums * ns;
    p.decay.resize((size_t)Nf);
    for (int64_t k = 0; k < Nf; ++k) p.decay[(size_t)k] = wwz_decay(c, f[k]);
    p.order.resize((size_t)Ntau);
    for (int64_t j = 0; j < Ntau; ++j) p.order[(size_t)j] = (int32_t)j;
    std::stable_sort(p.order.begin(), p.order.end(), [tau](int32_t a, int32_t b) { return tau[a] < tau[b]; });
    p.pos.resize((size_t)Ntau);
    p.tau_sorted.assign((size_t)(p.ngroups * p.TT), tau[p.order.back()]);
    for (int64_t q = 0; q < Ntau; ++q) {
        p.pos[(size_t)p.order[(size_t)q]] = (int32_t)q;
        p.tau_sorted[(size_t)q] = tau[p.order[(size_t)q]];
    }
    p.gmin.resize((size_t)p.ngroups); p.gmax.resize((size_t)p.ngroups);
    for (int64_t g = 0; g < p.ngroups; ++g) {
        p.gmin[(size_t)g] = p.tau_sorted[(size_t)(g * p.TT)];
        p.gmax[(size_t)g] = p.tau_sorted[(size_t)(g * p.TT + p.TT - 1)];
    }
    p.rmax.assign((size_t)p.ftiles, 0.0);
    for (int64_t k = 0; k < Nf; ++k) {
        double &r = p.rmax[(size_t)(k / kLombFreqTile)];
        if (radius[k] > r) r = radius[k];
    }
    p.status = kWwzOk;
    return p;
}

// ---- the work list: known once the device has found the samples of every (group, tile) ------------------------------------------------------
// A (group, tile) stages the samples with  gmin - rmax <= t <= gmax + rmax  (both edges formed in double as written; rounding is monotone,
// so every cell of the pair lies inside): the union over the group's times at the tile's largest radius.  edges[2 q], edges[2 q + 1] =
// #{t < lo}, #{t <= hi} of pair q = group ftiles + tile, from the device's binary search.  The range is cut at the absolute multiples of
// the slab length: one item per slab it touches, none for an empty range.
struct WwzItem {
    int32_t group = 0, tile = 0;
    int64_t first = 0, last = 0;        // its samples first .. last - 1 of the record
};
struct WwzWork {
    int status = kWwzUnsupported;
    std::string why;
    std::vector<WwzItem> items;
    std::vector<int64_t> offset;        // [pairs + 1]: the index of a pair's first item
    std::vector<int64_t> first_slab;    // [pairs]: the absolute index of the slab that item covers
    int64_t part_doubles = 0;           // items x rows x TT x 64
    double part_bytes = 0;
    double staged = 0, useful = 0;      // (sample, frequency, time) triples the kernel stages -- all 64 lanes and TT slots of every
                                        // item -- against those inside their cell: sum of count over the cells
};
inline WwzWork wwz_work(const WwzShape &sh, const std::vector<int64_t> &edges, double useful, int64_t max_items = kLombMaxGrid) {
    WwzWork w;
    const int64_t pairs = sh.ngroups * sh.ftiles, L = sh.slab_samples;
    double nitems = 0;                                                     // (counted before anything is laid out)
    for (int64_t q = 0; q < pairs; ++q) {
        const int64_t a = edges[(size_t)(2 * q)], b = edges[(size_t)(2 * q + 1)];
        if (b > a) nitems += (double)((b - 1) / L - a / L + 1);
    }
    if (nitems > (double)max_items) {
        w.why = "wwz: the work list (one item per group of times, tile of frequencies and slab of " + std::to_string((long long)L) + " samples) has " +
                std::to_string((long long)nitems) + " items, more than the " + std::to_string((long long)max_items) + " one launch takes";
        return w;
    }
    w.items.reserve((size_t)nitems); w.offset.reserve((size_t)pairs + 1); w.first_slab.reserve((size_t)pairs);
    for (int64_t q = 0; q < pairs; ++q) {
        const int64_t a = edges[(size_t)(2 * q)], b = edges[(size_t)(2 * q + 1)];
        w.offset.push_back((int64_t)w.items.size());
        w.first_slab.push_back(a / L);
        if (b <= a) continue;
        w.staged += (double)(b - a) * (double)(kLombFreqTile * sh.TT);
        for (int64_t s = a / L; s * L < b; ++s) {
            WwzItem it;
            it.group = (int32_t)(q / sh.ftiles); it.tile = (int32_t)(q % sh.ftiles);
            it.first = s * L > a ? s * L : a;
            it.last = (s + 1) * L < b ? (s + 1) * L : b;
            w.items.push_back(it);
        }
    }
    w.offset.push_back((int64_t)w.items.size());
    w.part_doubles = (int64_t)w.items.size() * sh.rows * sh.TT * kLombFreqTile;
    w.part_bytes = 8.0 * (double)w.part_doubles;
    w.useful = useful;
    w.status = kWwzOk;
    return w;
}

}  // namespace lpvs
