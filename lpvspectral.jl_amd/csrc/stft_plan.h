// stft_plan.h -- the host-side decisions of the STFT engine (spectrogram / melspectrogram / mfcc / welch_pgram / periodogram: melspec.hip;
// DESIGN.md 4.8, 4.10): the frames of a call, the FFT length and its split, the path, the frame pairs of a workgroup, the chunk of the
// four-step loop, the slabs of the frame average with the length of their sum chain, and the device memory all of it takes.
// Pure functions of numbers: melspec.hip allocates and launches what they say and computes none of this itself.
// No HIP dependency: the host-side test (tests/test_stft_plan.py) compiles it as it is.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "gram_form_plan.h"

namespace lpvs {

constexpr int kFftMax = 8192;        // complex points per workgroup (16 B each: 128 KiB of LDS)
constexpr int kThreads = 512;        // 8 waves: up to 256 VGPRs each, no spills in the radix-7 stage
constexpr int kMaxStages = 16;
constexpr int kMaxPairs = 512;       // frame pairs per workgroup (small nfft)
constexpr int kSplitPer = 10;        // split items per thread: pairs x bins of a workgroup <= kSplitPer * kThreads
constexpr int64_t kMaxLen = 1ll << 26;
constexpr size_t kScratchBudget = (size_t)1 << 30;   // bytes of four-step scratch per chunk of frame pairs
constexpr int64_t kWelchChain = 1024;        // most frames one workgroup adds sequentially into its slab (LDS paths)
constexpr int64_t kWelchSlabs = 1024;        // slabs launched when the frames allow it (more when kWelchChain asks for it)
constexpr int64_t kWelchChunkFrames = 256;   // frames per slab on the four-step paths
constexpr int64_t kWelchChunkPairs = kWelchChunkFrames / 2;
constexpr int64_t kWelchMaxSlabs = 1ll << 30;
constexpr size_t kComplexBytes = 16;         // one point of a spectrum (two doubles)

// ---- 7-smooth lengths and their factors ----------------------------------------------------------------------------------------------------
inline bool is_smooth(int64_t n) {
    if (n < 1) return false;
    for (int64_t p : {2, 3, 5, 7}) while (n % p == 0) n /= p;
    return n == 1;
}
inline int64_t next_smooth(int64_t n) {
    int64_t m = n < 1 ? 1 : n;
    while (!is_smooth(m)) ++m;
    return m;
}
struct Radices { int n = 0; int r[kMaxStages]; };
inline Radices factor(int64_t N) {
    Radices f;
    for (int p : {8, 4, 2, 3, 5, 7})
        while (N % p == 0) { f.r[f.n++] = p; N /= p; }
    return f;
}
// a length <= 2^26 the engine runs: <= 8192 in LDS, else n1 * n2 with both factors <= 8192 and the most balanced such split
struct FftSplit {
    int64_t len = 0, n1 = 0, n2 = 0;
    bool fits() const { return len > 0; }
};
inline FftSplit plan_length(int64_t N) {
    FftSplit p;
    if (!is_smooth(N) || N > kMaxLen) return p;
    if (N <= kFftMax) { p.len = N; p.n1 = N; p.n2 = 1; return p; }
    int64_t best = 0;
    for (int64_t d = 2; d <= kFftMax; ++d)
        if (N % d == 0 && N / d <= kFftMax && (best == 0 || std::llabs(d * d - N) < std::llabs(best * best - N))) best = d;
    if (best) { p.len = N; p.n1 = best; p.n2 = N / best; }
    return p;
}

// sequences of length N <= kFftMax one workgroup transforms at a time
inline int fft_batch(int64_t N) { return (int)std::max<int64_t>(1, kFftMax / N); }
// slabs a four-step chunk of nfr frames leaves (kWelchChunkPairs frame pairs each)
inline int64_t welch_chunk_slabs(int64_t nfr) { return ceil_div(nfr, kWelchChunkFrames); }

// ---- the plan of one call ------------------------------------------------------------------------------------------------------------------
// what the numbers refuse (the argument errors with their messages are melspec.hip's); a refused plan holds nothing behind the refusal
enum StftRefusal {
    kStftOk = 0,
    kStftNfftTooLong,        // nfft > 2^26
    kStftNoSplit,            // 7-smooth nfft > 8192 without two factors <= 8192
    kStftBluesteinTooLong,   // no 7-smooth m >= 2 nfft - 1 the engine runs up to 2^26
    kStftTooManySlabs,       // the frame average would need more than 2^30 slabs
    kStftWelchNoPair,        // the frame average on an LDS path without room for one frame pair (see `slabs`)
};
struct StftPlan {
    int kind = 0;
    bool welch = false, twosided = false;
    int64_t L = 0, n = 0, nfft = 0, nmels = 0, nmfcc = 0;
    // frames (DSP.arraysplit's) and outputs
    int64_t hop = 0, frames = 0, pairs = 0, nbins = 0, rows = 0, nout = 0;
    // the length: nfft, or the Bluestein length m (0 when nfft is 7-smooth)
    bool blue = false, lds = false;
    int64_t m = 0;
    FftSplit split;
    int path = 0;                        // 1 LDS, 2 four-step, 3 Bluestein in LDS, 4 Bluestein four-step
    // LDS paths: frame pairs per workgroup; 0 = the epilogue's regions do not fit next to one pair (`fallback` through global power columns)
    int64_t pairs_per_workgroup = 0;
    bool fallback = false;
    int fallback_batch = 0;              // ... whose FFT launch transforms this many pairs per workgroup
    int64_t chunk_pairs = 0;             // four-step paths: frame pairs per pass of the chunk loop
    // the frame average (0 for the other kinds)
    int64_t batches = 0;                 // LDS paths: workgroup batches of pairs_per_workgroup pairs
    int64_t slabs = 0, slab_frames = 0;  // S slabs of nbins partial sums, at most F frames behind one slab
    int64_t tree_depth = 0, sum_chain = 0;
    StftRefusal refusal = kStftOk;

    // ---- device memory: stft_device_bytes adds up these and nothing else, the allocations of melspec.hip ask for them by name
    size_t out_bytes(size_t elt) const { return elt * (size_t)nout; }          // the output staged on the device
    size_t signal_bytes(size_t elt) const { return elt * (size_t)L; }          // the signal staged on the device
    size_t slab_bytes() const { return sizeof(double) * (size_t)(slabs * nbins); }
    size_t flag_bytes() const { return sizeof(int32_t) * (size_t)frames; }     // frame flags; as many again of max-abs exponents
    size_t bluestein_bytes() const { return kComplexBytes * (size_t)m; }       // each of b, its transform and the four-step's scratch
    size_t pair_spectrum_bytes() const { return kComplexBytes * (size_t)split.len; }       // one frame pair's spectrum (as much again of scratch)
    size_t pair_power_bytes() const { return 2 * sizeof(double) * (size_t)nbins; }         // one frame pair's two power columns
    size_t fallback_power_bytes() const { return sizeof(double) * (size_t)(frames * nbins); }
    size_t fallback_spectra_bytes() const { return kComplexBytes * (size_t)(pairs * split.len); }
    bool flags_frames() const { return !lds || fallback; }                     // the sequences of these paths do not see whole frames
    bool power_columns() const { return kind != LPVS_STFT_POWER && !welch; }   // mel / MFCC beyond the LDS epilogue read power columns
};

inline StftPlan stft_plan(int kind, int64_t L, int64_t n, int64_t noverlap, int64_t nfft, int64_t nmels, int64_t nmfcc, bool twosided) {
    StftPlan p;
    p.kind = kind; p.welch = kind == LPVS_STFT_WELCH; p.twosided = twosided;
    p.L = L; p.n = n; p.nfft = nfft; p.nmels = nmels; p.nmfcc = nmfcc;
    p.hop = n - noverlap;
    p.frames = L >= n ? (L - n) / p.hop + 1 : 0;
    p.pairs = (p.frames + 1) / 2;
    p.nbins = nfft / 2 + 1;
    p.rows = p.welch ? (twosided ? nfft : p.nbins) : (kind == LPVS_STFT_POWER ? p.nbins : (kind == LPVS_STFT_MEL ? nmels : nmfcc));
    p.nout = p.welch ? p.rows : p.frames * p.rows;
    if (nfft > kMaxLen) { p.refusal = kStftNfftTooLong; return p; }
    // ---- the length: Bluestein on the smallest 7-smooth m >= 2 nfft - 1 the engine runs
    p.blue = !is_smooth(nfft);
    p.split = plan_length(nfft);
    if (p.blue) {
        p.m = next_smooth(2 * nfft - 1);
        while (p.m <= kMaxLen && !plan_length(p.m).fits()) p.m = next_smooth(p.m + 1);
        if (p.m > kMaxLen) { p.refusal = kStftBluesteinTooLong; return p; }
        p.split = plan_length(p.m);
    } else if (!p.split.fits()) {
        p.refusal = kStftNoSplit;
        return p;
    }
    const int64_t flen = p.split.len;
    p.lds = flen <= kFftMax;
    p.path = p.lds ? (p.blue ? 3 : 1) : (p.blue ? 4 : 2);
    if (p.frames == 0) return p;   // nothing runs: nothing to size
    if (p.lds) {
        // the FFT buffer, the power / mel / DCT regions of the epilogue (doubles) and the split's registers must fit
        const int64_t per_pair_dbl = kind == LPVS_STFT_POWER ? 0 : 2 * (p.nbins + nmels + (kind == LPVS_STFT_MFCC ? nmfcc : 0));
        int64_t b = kFftMax / flen;
        if (per_pair_dbl > 0) b = std::min<int64_t>(b, (2 * kFftMax) / per_pair_dbl);
        b = std::min<int64_t>(std::min<int64_t>(b, kMaxPairs), p.pairs);
        while (b > 1 && b * p.nbins > (int64_t)kSplitPer * kThreads) --b;
        p.pairs_per_workgroup = std::max<int64_t>(b, 0);
        p.fallback = p.pairs_per_workgroup < 1;
        if (p.fallback) p.fallback_batch = std::min<int>(fft_batch(flen), kMaxPairs);
    } else   // tmp + Z of a chunk within the scratch budget (at least one pair)
        p.chunk_pairs = std::max<int64_t>(1, std::min<int64_t>(p.pairs, (int64_t)(kScratchBudget / (2 * p.pair_spectrum_bytes()))));
    if (!p.welch) return p;
    // ---- the frame average.  LDS paths: workgroup g of S adds the power columns of the batches g, g + S, ... to slab g in ascending frame
    // order, at most kWelchChain frames; F is less the frames the last batch lacks when slab 0 holds it.  Four-step paths: every chunk is cut
    // in slabs of kWelchChunkFrames frames.  The slabs are then added in a pairwise tree: the longest chain of dependent additions behind one
    // bin is D = F - 1 + ceil(log2 S).
    if (p.lds) {
        // INVARIANT: pairs_per_workgroup >= 1 here.  The frame average has no mel or DCT region (its callers pass nmels = 0), so the
        // epilogue takes 2 nbins <= 2 kFftMax doubles per pair and one pair always fits; frames >= 1 was seen above.  Both divisions below
        // rest on it, and a caller who breaks it is refused rather than divided by zero.
        if (p.pairs_per_workgroup < 1) { p.refusal = kStftWelchNoPair; return p; }
        const int64_t b = p.pairs_per_workgroup;
        p.batches = ceil_div(p.pairs, b);
        const int64_t bpw = std::max<int64_t>(1, kWelchChain / (2 * b));
        p.slabs = std::max<int64_t>(std::min<int64_t>(p.batches, kWelchSlabs), ceil_div(p.batches, bpw));
        p.slab_frames = ceil_div(p.batches, p.slabs) * 2 * b - ((p.batches - 1) % p.slabs == 0 ? 2 * b * p.batches - p.frames : 0);
    } else
        for (int64_t p0 = 0; p0 < p.pairs; p0 += p.chunk_pairs) {
            const int64_t nfr = std::min<int64_t>(2 * std::min<int64_t>(p.chunk_pairs, p.pairs - p0), p.frames - 2 * p0);
            p.slabs += welch_chunk_slabs(nfr);
            p.slab_frames = std::max<int64_t>(p.slab_frames, std::min<int64_t>(nfr, kWelchChunkFrames));
        }
    if (p.slabs > kWelchMaxSlabs) { p.refusal = kStftTooManySlabs; return p; }
    while (((int64_t)1 << p.tree_depth) < p.slabs) ++p.tree_depth;
    p.sum_chain = p.slab_frames - 1 + p.tree_depth;
    return p;
}

// what a call needs of device memory before anything is allocated: the staged output and signal, the slabs, the minimum scratch (a chunk
// of one frame pair: its spectrum, as much again of scratch, its power columns), the Bluestein vectors, the frame flags and exponents, and
// the fallback's power columns and spectra of the whole call.  elt: bytes of an input / output element
inline size_t stft_device_bytes(const StftPlan &p, size_t elt, bool out_on_device, bool signal_on_device) {
    return (out_on_device ? 0 : p.out_bytes(elt)) + p.slab_bytes() + (signal_on_device ? 0 : p.signal_bytes(elt)) +
           (p.lds ? 0 : 2 * p.pair_spectrum_bytes()) + (p.power_columns() ? p.pair_power_bytes() : 0) + (p.blue ? 3 * p.bluestein_bytes() : 0) +
           (p.flags_frames() ? 2 * p.flag_bytes() : 0) + (p.fallback ? p.fallback_power_bytes() + p.fallback_spectra_bytes() : 0);
}

}  // namespace lpvs
