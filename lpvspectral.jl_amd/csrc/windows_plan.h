// windows_plan.h -- the host-side decisions of the batched-window engine (api.hip): how many windows share a pass, how a
// window range is cut into cache-sized chunks and parts, where the tile formats and max|M| live behind the packed inverses, and
// fourier2complex.  Pure functions of numbers: api.hip allocates and launches what they say and computes none of this itself.
// No HIP dependency: the host-side test (tests/test_windows_plan.py) compiles it as it is.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/lpvspectral.h"

namespace lpvs {

// ---- the packed inverse: tiles of 128 x 128, lower triangle ----------------------------------------------------------------------------
constexpr int64_t kTile = 128;
// bytes one mat-vec launch reads per tile: 36-bit fixed point (32-bit heads, a plane of nibbles, one step per row), its 32-bit reads
// (heads + steps: same slot layout, the nibble area is skipped), float head + 16-bit tail
constexpr size_t kMixedFixedTileBytes = 128 * 128 * 4 + 128 * 128 / 2 + 128 * 4, kMixedFloatTileBytes = 128 * 128 * 6;
constexpr size_t kMixedFixed32TileBytes = 128 * 128 * 4 + 128 * 4;
constexpr size_t kDiagFixedTileExtraBytes = 1024;       // a fixed-point tile on the diagonal (type 2) reads this much more

inline size_t packed_tiles(int64_t np) { const int64_t nblk = np / kTile; return (size_t)(nblk * (nblk + 1) / 2); }

// The buffer of nmat packed inverses of one size: nmat * packed_tiles * 128 * 128 elements of elt bytes, then one format byte per tile
// (rounded up to 256), then max|M| of every matrix (a single matrix leaves its largest row sum in the word after it).
struct PackedLayout {
    size_t tiles = 0;          // per matrix
    size_t elems_bytes = 0;    // = the offset of the tile-format bytes
    size_t types_bytes = 0;    // rounded
    size_t absmax_off = 0;
    size_t bytes = 0;          // of the whole buffer with formats and max|M| (without them: elems_bytes)
};
inline PackedLayout packed_layout(int64_t np, size_t elt, size_t nmat) {
    PackedLayout l;
    l.tiles = packed_tiles(np);
    l.elems_bytes = elt * l.tiles * (size_t)(kTile * kTile) * nmat;
    l.types_bytes = (l.tiles * nmat + 255) / 256 * 256;
    l.absmax_off = l.elems_bytes + l.types_bytes;
    l.bytes = l.absmax_off + (8 * nmat > 256 ? 8 * nmat : 256);
    return l;
}

struct TileCensus { size_t fixed = 0, diag = 0, total = 0; };   // fixed-point tiles (format != 0), of which on the diagonal (format 2), all
inline TileCensus tile_census(const unsigned char *types, size_t count) {
    TileCensus c;
    c.total = count;
    for (size_t i = 0; i < count; ++i) { c.fixed += types[i] != 0; c.diag += types[i] == 2; }
    return c;
}
// bytes of packed inverse one mat-vec launch streams (read32: the fixed-point tiles without their nibble planes)
inline double census_stream_bytes(const TileCensus &c, bool read32) {
    return (double)c.fixed * (double)(read32 ? kMixedFixed32TileBytes : kMixedFixedTileBytes) + (double)c.diag * (double)kDiagFixedTileExtraBytes +
           (double)(c.total - c.fixed) * (double)kMixedFloatTileBytes;
}

// ---- the pass plan -----------------------------------------------------------------------------------------------------------------------
constexpr size_t kPanelBudgetBytes = (size_t)48 << 30;    // k-major regressor panels of one pass (dense form); LPVS_BATCH_PANEL_GIB
constexpr size_t kMatrixBudgetBytes = (size_t)32 << 30;   // resident np x np matrices of one pass (structured form)
constexpr int64_t kMaxWindowsPerPass = 8192;
constexpr int64_t kSegmentSamples = 4096;                 // structured form: samples per segment of a window
// the sample split of the dense form is chosen for this many windows, whatever the shard holds: the summation order of a window must
// not depend on how the windows are sharded
constexpr int64_t kNominalBatch = 64;

inline int64_t fourier_regressors(int64_t Nf, bool zerofreq) { return zerofreq ? 2 * Nf - 1 : 2 * Nf; }   // cos and sin columns; no sine at f = 0

struct WinPassPlan {
    int64_t nreg = 0, np = 0, ld = 0;   // regressors, padded to 128 (matrices, vectors), to 256 (panel rows)
    int nmat = 0;                       // resident np x np matrices per window
    int64_t windows = 0;                // per pass
    int64_t nrows = 0;                  // samples per window as stored: n (structured), the Gram plan's padded rows (dense form)
    size_t panel_bytes = 0;             // per window (structured: none)
    int64_t seg_len = 0; int segs = 0;  // structured form only
    size_t vb = 0;                      // bytes of one state vector of a pass: [windows * ns][np] doubles
};
// dense_rows: ksplit * rows_per_chunk of the dense form's Gram plan for (nreg, n, kNominalBatch); unread when structured
inline WinPassPlan window_pass_plan(int64_t n, int64_t Nf, bool zerofreq, int64_t ns, int64_t nwin, bool sparse, bool init, bool structured,
                                    int64_t dense_rows, size_t panel_budget) {
    const auto up = [](int64_t a, int64_t b) { return (a + b - 1) / b * b; };
    WinPassPlan p;
    p.nreg = fourier_regressors(Nf, zerofreq); p.np = up(p.nreg, 128); p.ld = up(p.nreg, 256);
    // sparse: M and its packed copy; dense: Q, M and the inverse's work space; init: A'A and its inverse besides
    p.nmat = (sparse ? 2 : 3) + (init ? 2 : 0);
    p.nrows = structured ? n : dense_rows;
    p.panel_bytes = structured ? 0 : sizeof(double) * (size_t)p.nrows * (size_t)p.ld;
    // One rule: what the budget holds -- the matrices of a structured pass, the panels of a dense-form one at their nominal row count
    // round_up(n, 64) -- between 1 and min(nwin, 8192); then the dense form's true panels (the Gram plan pads the rows further).
    const size_t first = structured ? kMatrixBudgetBytes / (sizeof(double) * (size_t)p.np * (size_t)p.np * (size_t)p.nmat)
                                    : panel_budget / (sizeof(double) * (size_t)up(n, 64) * (size_t)p.ld);
    const int64_t most = nwin < kMaxWindowsPerPass ? nwin : kMaxWindowsPerPass;
    p.windows = first < 1 ? 1 : ((int64_t)first > most ? most : (int64_t)first);
    if (!structured && p.panel_bytes * (size_t)p.windows > panel_budget) {
        const int64_t fit = (int64_t)(panel_budget / p.panel_bytes);
        p.windows = fit < 1 ? 1 : fit;
    }
    // the segment length is fixed: the summation order of a window must not depend on how many windows share the pass, so that window
    // shards (ranks of a node) reproduce the whole run bit for bit
    p.seg_len = structured ? (n < kSegmentSamples ? n : kSegmentSamples) : 0;
    p.segs = structured ? (int)((n + p.seg_len - 1) / p.seg_len) : 0;
    p.vb = sizeof(double) * (size_t)p.np * (size_t)(p.windows * ns);
    return p;
}

// ---- the chunk plan ------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMinChunkWindows = 16;       // the least chunk, and the least part of one
constexpr int64_t kMinChunkIters = 64;         // shorter runs are not worth the threads
constexpr double kCacheFill = 1.0625;          // default chunk: this much of the Infinity Cache (285 MB of 256 MiB; measured: api.hip)
constexpr int kDefaultInFlight = 2;

struct WinChunkPlan {
    bool chunked = false;      // false: the uncut engine takes the whole range
    int64_t chunk = 0;         // windows per chunk, even over the range (the last one may be shorter)
    int in_flight = 0;
    // parts of a chunk of cw windows, and the window range [lo, hi) of part p relative to the chunk's first window
    int parts(int64_t cw) const { return cw >= kMinChunkWindows * in_flight ? in_flight : 1; }
    static int64_t part_lo(int64_t cw, int parts, int p) { return cw * p / parts; }
    static int64_t part_hi(int64_t cw, int parts, int p) { return cw * (p + 1) / parts; }
};
// Does a range go to the chunked engine at all?  Not a dense estimate, not a handful of windows or iterations, not one part without a chunk
// size.  (Asked on its own before the frequency grid is looked at: np is not needed.)
inline bool window_chunking_applies(int64_t nwin, int64_t iters, bool sparse, int opt_chunk_mb, int opt_in_flight) {
    const bool one_part = opt_in_flight == 1, no_chunk_size = opt_chunk_mb == LPVS_WINDOW_UNCUT;
    return sparse && nwin >= kMinChunkWindows && iters >= kMinChunkIters && !(one_part && no_chunk_size);
}
// opt_chunk_mb, opt_in_flight: LPVS_OPT_WINDOW_CHUNK_MB and LPVS_OPT_WINDOWS_IN_FLIGHT as option_in_effect answers (0: the defaults)
inline WinChunkPlan window_chunk_plan(int64_t nwin, int64_t ns, int64_t np, int64_t iters, bool sparse, int opt_chunk_mb, int opt_in_flight,
                                      double cache_bytes) {
    WinChunkPlan c;
    const double chunk_mb = opt_chunk_mb == LPVS_WINDOW_UNCUT ? 0.0 : (opt_chunk_mb > 0 ? (double)opt_chunk_mb : kCacheFill * cache_bytes * 1e-6);
    c.in_flight = opt_in_flight > 0 ? opt_in_flight : kDefaultInFlight;
    c.chunked = window_chunking_applies(nwin, iters, sparse, opt_chunk_mb, opt_in_flight);
    if (!c.chunked) return c;
    // a window weighs its packed inverse with every tile fixed point, once per signal
    const double win_bytes = (double)packed_tiles(np) * (double)kMixedFixedTileBytes * (double)ns;
    int64_t chunk = chunk_mb > 0 ? (int64_t)(chunk_mb * 1e6 / win_bytes) : nwin;
    if (chunk < kMinChunkWindows) chunk = kMinChunkWindows;
    if (chunk > nwin) chunk = nwin;
    const int64_t nchunks = (nwin + chunk - 1) / chunk;
    c.chunk = (nwin + nchunks - 1) / nchunks;
    return c;
}

// ---- fourier2complex (src/utilities.jl:62-73): [cos coefficients; sin coefficients (none at f = 0)] -> re, im of Nf frequencies ---------
inline void fourier2complex(const double *c, int64_t Nf, bool zerofreq, double *re, double *im) {
    if (!zerofreq) for (int64_t i = 0; i < Nf; ++i) { re[i] = c[i]; im[i] = c[Nf + i]; }
    else { re[0] = c[0]; im[0] = 0.0; for (int64_t i = 1; i < Nf; ++i) { re[i] = c[i]; im[i] = c[Nf + i - 1]; } }
}

}  // namespace lpvs
