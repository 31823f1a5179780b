// nufft_bins.h -- the index arithmetic of the gather-form spreading ("gather spreading"): which sorted samples touch a
// cell, which kernel value of a sample a cell takes, how a launch is cut into workgroups and how the work buffer is carved up.
// nufft.hip launches what this header says and decides nothing more.  No HIP dependency: the host-side test
// (tests/test_nufft_bins.py) compiles it as it is and runs an integer model of both spreadings against it.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LPVS_NU_HD __host__ __device__
#else
#define LPVS_NU_HD
#endif

namespace lpvs {

constexpr int kNuWidth = 16;          // kernel width w: a sample with first cell cell0 touches cells cell0 .. cell0 + 15 (cyclically)
constexpr int kNuChunk = 32768;       // samples per chunk partial (the `partial` layout nufft_reduce_kernel sums over)
constexpr int kNuBinChunk = 4096;     // samples sorted together by cell0: a chunk is kNuChunk / kNuBinChunk sorted runs
constexpr int kNuCellBlock = 256;     // consecutive cells per gather workgroup, one per thread (nf is a power of two >= 256)
constexpr int kNuGatherGrids = 8;     // grids (4 weight columns, plain + twin) a gather thread accumulates in registers
constexpr int kNuStage = 512;         // sorted positions staged in LDS at a time (cell0, sample index, 8 weights in quanta: 36 KB)

// grids per SCATTER workgroup (LDS grids of nf 64-bit cells); also what fixes the padded grid count of the `partial` layout
LPVS_NU_HD inline int nu_scatter_gpw(int nf) { return nf <= 4096 ? 4 : 2; }

// ---- which sorted positions touch a block of cells ----------------------------------------------------------------------------------
// bin_start[0 .. nf] is the exclusive scan of a sorted run's histogram over cell0: the samples with cell0 == b sit at the sorted
// positions bin_start[b] .. bin_start[b + 1].  Cells first .. first + count - 1 (no wrap: first + count <= nf) are touched by the bins
// first - 15 .. first + count - 1, cyclically: ONE contiguous range of positions, or TWO where the bins wrap below cell 0.  A block
// that the bins go all the way round (count + 15 >= nf) takes the whole run once.  Empty ranges have lo == hi.
struct NuRange { int lo, hi; };
struct NuRanges { NuRange r[2]; };
template <class BinStart>
LPVS_NU_HD inline NuRanges nu_cell_ranges(const BinStart &bin_start, int nf, int first, int count) {
    NuRanges o;
    const int b0 = first - (kNuWidth - 1);
    if (count + (kNuWidth - 1) >= nf) { o.r[0] = {bin_start[0], bin_start[nf]}; o.r[1] = {0, 0}; }
    else if (b0 >= 0) { o.r[0] = {bin_start[b0], bin_start[first + count]}; o.r[1] = {0, 0}; }
    else { o.r[0] = {bin_start[b0 + nf], bin_start[nf]}; o.r[1] = {bin_start[0], bin_start[first + count]}; }
    return o;
}
// the kernel value cell c takes from a sample whose support starts at cell0: taps[16 s + k], k = (c - cell0) mod nf  (< 16 for every
// sample of nu_cell_ranges(.., c, 1))
LPVS_NU_HD inline int nu_tap_index(int c, int cell0, int nf) { return (c - cell0) & (nf - 1); }

// ---- how a launch is cut ----------------------------------------------------------------------------------------------------------
// A gather workgroup = (chunk, block of kNuCellBlock cells, group of kNuGatherGrids grids).  Consecutive workgroup ids go round the
// eight XCDs; the groups of one (chunk, cell block) follow each other on ONE XCD, so the kernel values of that block's samples are
// fetched into one L2 and found there by the other groups.
struct NuGatherPlan {
    int nchunks, nbinchunks, ncellblocks, ngroups;   // chunks of kNuChunk, sorted runs of kNuBinChunk, nf / 256, ceil(2 nq / 8)
    int padded_grids;                                // grids per chunk in `partial`: 2 nq rounded up to the scatter group
    int64_t nblocks;                                 // workgroups launched (a multiple of 8; ids past the work return at once)
};
LPVS_NU_HD inline NuGatherPlan nu_gather_plan(int64_t N, int nf, int nq) {
    NuGatherPlan p;
    const int gpw = nu_scatter_gpw(nf);
    p.nchunks = (int)((N + kNuChunk - 1) / kNuChunk);
    p.nbinchunks = (int)((N + kNuBinChunk - 1) / kNuBinChunk);
    p.ncellblocks = nf / kNuCellBlock;
    p.ngroups = (2 * nq + kNuGatherGrids - 1) / kNuGatherGrids;
    p.padded_grids = (2 * nq + gpw - 1) / gpw * gpw;
    const int64_t units = (int64_t)p.nchunks * p.ncellblocks;
    p.nblocks = 8 * (int64_t)p.ngroups * ((units + 7) / 8);
    return p;
}
struct NuGatherBlock { int chunk, cellblock, group; bool valid; };
LPVS_NU_HD inline NuGatherBlock nu_gather_block(const NuGatherPlan &p, int64_t block) {
    const int xcd = (int)(block & 7);
    const int64_t jj = block >> 3;
    const int64_t unit = xcd + 8 * (jj / p.ngroups);          // (chunk, cell block), cell blocks fastest
    NuGatherBlock b;
    b.group = (int)(jj % p.ngroups);
    b.valid = unit < (int64_t)p.nchunks * p.ncellblocks;
    b.chunk = (int)(unit / p.ncellblocks);
    b.cellblock = (int)(unit % p.ncellblocks);
    return b;
}

// ---- the work buffer ----------------------------------------------------------------------------------------------------------------
// Byte offsets.  What depends on (N, nf) only -- the coordinates and their binning -- is at the head, so that a later call with other
// weights (reuse_coords) finds it in place whatever its nq.
struct NuWork {
    size_t taps, cell0, perm, bin_start, partial, scale, invq, grid, colmax, total;
};
inline size_t nu_align256(size_t b) { return (b + 255) / 256 * 256; }
inline NuWork nu_work_layout(int64_t N, int nf, int64_t nslots, int64_t nq) {
    const NuGatherPlan p = nu_gather_plan(N, nf, (int)nq);
    NuWork w;
    size_t b = 0;
    w.taps = b;      b += nu_align256(sizeof(double) * (size_t)N * kNuWidth);                                      // [N][16] kernel values
    w.cell0 = b;     b += nu_align256(sizeof(int) * (size_t)N);                                                    // [N] first cell
    w.perm = b;      b += nu_align256(sizeof(int) * (size_t)N);                                                    // [N] sample (run-local) at a sorted position
    w.bin_start = b; b += nu_align256(sizeof(int) * (size_t)p.nbinchunks * (size_t)(nf + 1));                      // [runs][nf + 1]
    w.partial = b;   b += nu_align256(sizeof(long long) * (size_t)p.nchunks * (size_t)p.padded_grids * (size_t)nf);   // chunk partial grids
    w.scale = b;     b += nu_align256(sizeof(double) * (size_t)(2 * nq) * (size_t)nslots);                         // quantum / phihat
    w.invq = b;      b += nu_align256(sizeof(double) * (size_t)(2 * nq));                                          // 1 / quantum
    w.grid = b;      b += nu_align256(sizeof(double) * (size_t)(2 * nq) * (size_t)nf);                             // reduced grids
    w.colmax = b;    b += nu_align256(sizeof(unsigned long long) * (size_t)nq);                                    // column maxima
    w.total = b;
    return w;
}

}  // namespace lpvs
