"""The index arithmetic of the gather-form NUFFT spreading (csrc/nufft_bins.h).  The header has no HIP dependency: a
small host program is built against it with -fsanitize=address,undefined and run directly; CPU only.

    1  an integer model of both spreadings -- the scatter (every sample adds its 16 addends to the cells cell0 .. cell0 + 15) and the
       gather exactly as nufft_gather_kernel walks it (sorted runs, cell blocks, staged tiles, per-cell ranges, tap index) -- over random
       64-bit "addends": the chunk partials must be EQUAL, every addend taken exactly once
    2  the range split of a cell and of a cell block against literals worked by hand
    3  the work-buffer carve-up: aligned, in order, without overlap, its head independent of the number of weight vectors"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

PROGRAM = r"""
#include "nufft_bins.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace lpvs;
typedef unsigned long long u64;
static u64 mix(u64 v) { v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull; v ^= v >> 33; return v; }
static u64 addend(long s, int k, int grid) { return mix((u64)s * 64 + (u64)k * 4 + (u64)grid + 0x9e3779b97f4a7c15ull); }

// kind: 0 uniform, 1 every support wraps (cell0 >= nf - 15), 2 few occupied cells (most bins empty), 3 all samples in ONE cell
static int model(int nf, long N, int kind, int nq) {
    std::vector<int> cell0((size_t)N);
    u64 r = mix((u64)nf * 1315423911ull + (u64)N * 2654435761ull + (u64)kind);
    for (long s = 0; s < N; ++s) {
        r = mix(r + 1);
        if (kind == 0) cell0[(size_t)s] = (int)(r % (u64)nf);
        else if (kind == 1) cell0[(size_t)s] = nf - 15 + (int)(r % 15);
        else if (kind == 2) cell0[(size_t)s] = (int)((r % 7) * (u64)(nf / 7 + 1)) % nf;
        else cell0[(size_t)s] = nf - 3;
    }
    const NuGatherPlan plan = nu_gather_plan(N, nf, nq);
    const int ngrids = 2 * nq;
    std::vector<u64> scatter((size_t)plan.nchunks * ngrids * nf, 0), gather(scatter.size(), 0);
    for (long s = 0; s < N; ++s)
        for (int k = 0; k < kNuWidth; ++k)
            for (int g = 0; g < ngrids; ++g)
                scatter[((size_t)(s / kNuChunk) * ngrids + g) * nf + (size_t)((cell0[(size_t)s] + k) & (nf - 1))] += addend(s, k, g);
    // the binning, as nufft_bin_kernel does it
    std::vector<int> bin_start((size_t)plan.nbinchunks * (nf + 1)), perm((size_t)N);
    for (int run = 0; run < plan.nbinchunks; ++run) {
        const long base = (long)run * kNuBinChunk, count = N - base < kNuBinChunk ? N - base : kNuBinChunk;
        std::vector<int> cnt((size_t)nf, 0);
        for (long i = 0; i < count; ++i) ++cnt[(size_t)cell0[(size_t)(base + i)]];
        int *bs = &bin_start[(size_t)run * (nf + 1)];
        int acc = 0;
        for (int b = 0; b < nf; ++b) { bs[b] = acc; acc += cnt[(size_t)b]; cnt[(size_t)b] = bs[b]; }
        bs[nf] = acc;
        for (long i = count - 1; i >= 0; --i) perm[(size_t)(base + cnt[(size_t)cell0[(size_t)(base + i)]]++)] = (int)i;   // (any order inside a bin)
    }
    // the gather, workgroup by workgroup as nufft_gather_kernel walks it
    std::vector<int> visited((size_t)plan.nchunks * plan.ncellblocks * plan.ngroups, 0);
    const int runs = kNuChunk / kNuBinChunk;
    for (long blk = 0; blk < plan.nblocks; ++blk) {
        const NuGatherBlock b = nu_gather_block(plan, blk);
        if (!b.valid) continue;
        if (b.chunk < 0 || b.chunk >= plan.nchunks || b.cellblock < 0 || b.cellblock >= plan.ncellblocks || b.group < 0 || b.group >= plan.ngroups) return 10;
        ++visited[((size_t)b.chunk * plan.ncellblocks + b.cellblock) * plan.ngroups + b.group];
        for (int sub = 0; sub < runs; ++sub) {
            const long run = (long)b.chunk * runs + sub, base = run * kNuBinChunk;
            if (base >= N) break;
            const int *bs = &bin_start[(size_t)run * (nf + 1)];
            const NuRanges block = nu_cell_ranges(bs, nf, b.cellblock * kNuCellBlock, kNuCellBlock);
            for (int seg = 0; seg < 2; ++seg)
                for (int t0 = block.r[seg].lo; t0 < block.r[seg].hi; t0 += kNuStage) {
                    const int t1 = t0 + kNuStage < block.r[seg].hi ? t0 + kNuStage : block.r[seg].hi;
                    for (int t = 0; t < kNuCellBlock; ++t) {
                        const int c = b.cellblock * kNuCellBlock + t;
                        const NuRanges mine = nu_cell_ranges(bs, nf, c, 1);
                        for (int rr = 0; rr < 2; ++rr) {
                            const int lo = mine.r[rr].lo > t0 ? mine.r[rr].lo : t0, hi = mine.r[rr].hi < t1 ? mine.r[rr].hi : t1;
                            for (int p = lo; p < hi; ++p) {
                                if (p - t0 < 0 || p - t0 >= kNuStage) return 11;              // outside the staged tile
                                const long s = base + perm[(size_t)(base + p)];
                                const int k = nu_tap_index(c, cell0[(size_t)s], nf);
                                if (k < 0 || k >= kNuWidth) return 12;                       // a sample that does not touch this cell
                                for (int gi = 0; gi < kNuGatherGrids; ++gi) {
                                    const int g = b.group * kNuGatherGrids + gi;
                                    if (g < ngrids) gather[((size_t)b.chunk * ngrids + g) * nf + (size_t)c] += addend(s, k, g);
                                }
                            }
                        }
                    }
                }
        }
    }
    for (int v : visited) if (v != 1) return 13;
    if (plan.nblocks % 8 != 0) return 14;
    return memcmp(scatter.data(), gather.data(), sizeof(u64) * scatter.size()) == 0 ? 0 : 1;
}

struct Lin { int step; int operator[](int b) const { return step * b; } };   // bin_start[b] = step * b: `step` samples in every bin

int main(int argc, char **argv) {
    if (argc >= 2 && strcmp(argv[1], "model") == 0) {
        if (argc < 6) return 2;
        const int rc = model(atoi(argv[2]), atol(argv[3]), atoi(argv[4]), atoi(argv[5]));
        printf("model=%d\n", rc);
        return 0;
    }
    if (argc >= 2 && strcmp(argv[1], "ranges") == 0) {
        if (argc < 6) return 2;
        const NuRanges r = nu_cell_ranges(Lin{atoi(argv[2])}, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
        printf("%d %d %d %d\n", r.r[0].lo, r.r[0].hi, r.r[1].lo, r.r[1].hi);
        return 0;
    }
    if (argc >= 2 && strcmp(argv[1], "tap") == 0) {
        if (argc < 5) return 2;
        printf("%d\n", nu_tap_index(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
        return 0;
    }
    if (argc >= 2 && strcmp(argv[1], "work") == 0) {
        if (argc < 6) return 2;
        const long N = atol(argv[2]); const int nf = atoi(argv[3]); const long nslots = atol(argv[4]), nq = atol(argv[5]);
        const NuWork w = nu_work_layout(N, nf, nslots, nq);
        const NuGatherPlan p = nu_gather_plan(N, nf, (int)nq);
        printf("taps=%zu cell0=%zu perm=%zu bin_start=%zu partial=%zu scale=%zu invq=%zu grid=%zu colmax=%zu total=%zu nchunks=%d nbinchunks=%d "
               "ncellblocks=%d ngroups=%d padded_grids=%d nblocks=%lld\n", w.taps, w.cell0, w.perm, w.bin_start, w.partial, w.scale, w.invq, w.grid,
               w.colmax, w.total, p.nchunks, p.nbinchunks, p.ncellblocks, p.ngroups, p.padded_grids, (long long)p.nblocks);
        return 0;
    }
    return 2;
}
"""


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def bins(tmp_path_factory):
    """bins(*args) -> the output line of the host program (a stand-alone executable under AddressSanitizer and UBSan)."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("nufft_bins")
    src, exe = os.path.join(d, "nufft_bins_model.cpp"), os.path.join(d, "nufft_bins_model")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-x", "c++",
                           "-I", HEADER_DIR, src, "-o", exe])   # (host only: the header must not need the HIP runtime)

    def run(*args):
        return subprocess.check_output([exe] + [str(a) for a in args], text=True).strip()
    yield run
    shutil.rmtree(d, ignore_errors=True)


CHUNK = 32768
KINDS = {"uniform": 0, "wrapping": 1, "empty_bins": 2, "one_bin": 3}


@pytest.mark.parametrize("nf", [256, 4096, 8192])
@pytest.mark.parametrize("kind", list(KINDS))
def test_gather_model_equals_scatter_model(bins, nf, kind):
    """One sample, a ragged last run (5000 = 4096 + 904), 4096, chunk + 1 (one sample in a second chunk), 2 chunk - 1 (ragged last chunk);
    three weight vectors = six grids: one group of eight with two idle grids; five vectors = ten grids: a second, ragged group."""
    for N, nq in ((1, 3), (5000, 5), (4096, 3), (CHUNK + 1, 1), (2 * CHUNK - 1, 1)):
        assert bins("model", nf, N, KINDS[kind], nq) == "model=0", (nf, kind, N, nq)


def test_range_split_against_hand_worked_literals(bins):
    """bin_start[b] = 3 b (three samples in every bin).  Cell c takes the bins c - 15 .. c."""
    def r(step, nf, first, count):
        return tuple(int(v) for v in bins("ranges", step, nf, first, count).split())
    nf = 256
    assert r(3, nf, 0, 1) == (3 * 241, 3 * 256, 0, 3)            # c = 0: bins 241 .. 255, then bin 0
    assert r(3, nf, 14, 1) == (3 * 255, 3 * 256, 0, 3 * 15)      # c = 14: bin 255, then bins 0 .. 14
    assert r(3, nf, 15, 1) == (0, 3 * 16, 0, 0)                  # c = 15: bins 0 .. 15, no wrap
    assert r(3, nf, nf - 1, 1) == (3 * 240, 3 * 256, 0, 0)       # c = nf - 1: bins 240 .. 255
    assert r(3, 4096, 4095, 1) == (3 * 4080, 3 * 4096, 0, 0)
    assert r(3, 4096, 0, 1) == (3 * 4081, 3 * 4096, 0, 3)
    # blocks of 256 cells: the whole run once when the bins go all the way round, two ranges for the first block otherwise
    assert r(3, 256, 0, 256) == (0, 3 * 256, 0, 0)
    assert r(3, 4096, 0, 256) == (3 * 4081, 3 * 4096, 0, 3 * 256)
    assert r(3, 4096, 256, 256) == (3 * 241, 3 * 512, 0, 0)
    assert r(3, 8192, 7936, 256) == (3 * 7921, 3 * 8192, 0, 0)
    # the kernel value a cell takes: k = (c - cell0) mod nf
    assert [int(bins("tap", *a)) for a in ((5, 5, 256), (20, 5, 256), (0, 250, 256), (3, 4090, 4096), (8191, 8176, 8192))] == [0, 15, 6, 9, 15]


def test_work_buffer_carve_up(bins):
    def layout(N, nf, nslots, nq):
        return {k: int(v) for k, v in (kv.split("=") for kv in bins("work", N, nf, nslots, nq).split())}
    order = ["taps", "cell0", "perm", "bin_start", "partial", "scale", "invq", "grid", "colmax"]
    for N, nf, nslots, nq in ((1 << 20, 4096, 1032, 36), (1 << 20, 4096, 344, 8), (4096, 256, 64, 1), (9000, 8192, 2008, 3), (70001, 2048, 500, 10)):
        w = layout(N, nf, nslots, nq)
        gpw = 4 if nf <= 4096 else 2
        nchunks, nruns = -(-N // CHUNK), -(-N // 4096)
        padded = -(-2 * nq // gpw) * gpw
        assert (w["nchunks"], w["nbinchunks"], w["ncellblocks"], w["ngroups"], w["padded_grids"]) == (nchunks, nruns, nf // 256, -(-2 * nq // 8), padded)
        assert w["nblocks"] == 8 * w["ngroups"] * -(-(nchunks * (nf // 256)) // 8)
        need = dict(taps=8 * 16 * N, cell0=4 * N, perm=4 * N, bin_start=4 * nruns * (nf + 1), partial=8 * nchunks * padded * nf, scale=8 * 2 * nq * nslots,
                    invq=8 * 2 * nq, grid=8 * 2 * nq * nf, colmax=8 * nq)
        assert w["taps"] == 0
        for a, b in zip(order, order[1:] + ["total"]):
            assert w[a] % 256 == 0 and w[b] % 256 == 0
            assert w[a] + need[a] <= w[b] < w[a] + need[a] + 256, (a, b)       # no overlap, no more than the alignment between them
    # the coordinates and their binning do not move with the number of weight vectors (reuse_coords), and the Gram's buffer holds a rhs call
    big, small = layout(1 << 20, 4096, 1032, 36), layout(1 << 20, 4096, 344, 8)
    assert all(big[k] == small[k] for k in ("taps", "cell0", "perm", "bin_start", "partial"))
    assert small["total"] <= big["total"]
