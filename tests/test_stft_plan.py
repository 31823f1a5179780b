"""What the STFT engine decides on the host (csrc/stft_plan.h): the frames of a call, the FFT length and its split,
the path, the frame pairs of a workgroup, the chunk of the four-step loop, the slabs of the frame average with their sum chain, the
refusals, and the device memory a call asks for.  The header has no HIP dependency: a tiny host program is built against it and prints
what it decides; CPU only.  Every expected value below is a literal worked from the rules, none is computed by asking the header a
second way.

    1  spectrogram / mel / MFCC: frames, path, pairs per workgroup, the fallback, Bluestein lengths, chunks
    2  splits and refusals
    3  the frame average: slabs and sum chain on named cases, the bound D <= 1100 over a seeded sweep
    4  device memory, term by term"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: stft_plan_dump plan|bytes|split|chains NUMBER ...  ->  lines of key=value pairs
PROGRAM = r"""
#include "stft_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
static lpvs::StftPlan plan_of(const long long *v) { return lpvs::stft_plan((int)v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] != 0); }
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<long long> v;
    for (int i = 2; i < argc; ++i) v.push_back(atoll(argv[i]));
    if (!strcmp(argv[1], "plan")) {            // kind L n noverlap nfft nmels nmfcc twosided
        if (v.size() != 8) return 2;
        const lpvs::StftPlan p = plan_of(v.data());
        printf("hop=%lld frames=%lld pairs=%lld nbins=%lld rows=%lld nout=%lld blue=%d lds=%d m=%lld len=%lld n1=%lld n2=%lld path=%d "
               "pairs_per_workgroup=%lld fallback=%d fallback_batch=%d chunk_pairs=%lld batches=%lld slabs=%lld slab_frames=%lld tree_depth=%lld "
               "sum_chain=%lld refusal=%d\n", (long long)p.hop, (long long)p.frames, (long long)p.pairs, (long long)p.nbins, (long long)p.rows,
               (long long)p.nout, (int)p.blue, (int)p.lds, (long long)p.m, (long long)p.split.len, (long long)p.split.n1, (long long)p.split.n2,
               p.path, (long long)p.pairs_per_workgroup, (int)p.fallback, p.fallback_batch, (long long)p.chunk_pairs, (long long)p.batches,
               (long long)p.slabs, (long long)p.slab_frames, (long long)p.tree_depth, (long long)p.sum_chain, (int)p.refusal);
    } else if (!strcmp(argv[1], "bytes")) {    // the plan's eight, then elt out_on_device signal_on_device
        if (v.size() != 11) return 2;
        printf("bytes=%zu\n", lpvs::stft_device_bytes(plan_of(v.data()), (size_t)v[8], v[9] != 0, v[10] != 0));
    } else if (!strcmp(argv[1], "split")) {    // N
        if (v.size() != 1) return 2;
        const lpvs::FftSplit s = lpvs::plan_length(v[0]);
        long long prod = 1;                    // of the radices of n1's stages (a length that does not fit has none)
        if (s.fits()) {
            const lpvs::Radices r = lpvs::factor(s.n1);
            for (int i = 0; i < r.n; ++i) prod *= r.r[i];
        }
        printf("fits=%d len=%lld n1=%lld n2=%lld smooth=%d radix_product=%lld\n", (int)s.fits(), (long long)s.len, (long long)s.n1, (long long)s.n2,
               (int)lpvs::is_smooth(v[0]), prod);
    } else if (!strcmp(argv[1], "chains")) {   // frame averages: L n noverlap nfft, any number of times -> a line each
        if (v.size() % 4) return 2;
        for (size_t i = 0; i < v.size(); i += 4) {
            const lpvs::StftPlan p = lpvs::stft_plan(LPVS_STFT_WELCH, v[i], v[i + 1], v[i + 2], v[i + 3], 0, 0, false);
            printf("frames=%lld path=%d pairs_per_workgroup=%lld sum_chain=%lld slabs=%lld refusal=%d\n", (long long)p.frames, p.path,
                   (long long)p.pairs_per_workgroup, (long long)p.sum_chain, (long long)p.slabs, (int)p.refusal);
        }
    } else return 2;
    return 0;
}
"""

POWER, MEL, MFCC, WELCH = 1, 2, 3, 4                       # LPVS_STFT_* of include/lpvspectral.h
OK, NFFT_TOO_LONG, NO_SPLIT, BLUESTEIN_TOO_LONG, TOO_MANY_SLABS, WELCH_NO_PAIR = range(6)   # StftRefusal


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(mode, numbers...) -> the dict of integers the program prints (a list of them for the modes that print several lines)."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("stft_plan")
    src, exe = os.path.join(d, "stft_plan_dump.cpp"), os.path.join(d, "stft_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(mode, *numbers):
        out = subprocess.check_output([exe, mode] + [str(int(x)) for x in numbers], text=True)
        rows = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in out.splitlines()]
        return rows if mode == "chains" else rows[0]
    yield run
    shutil.rmtree(d, ignore_errors=True)


def plan(dump, kind, L, n, noverlap, nfft, *, nmels=0, nmfcc=0, twosided=0):
    return dump("plan", kind, L, n, noverlap, nfft, nmels, nmfcc, twosided)


def nbytes(dump, kind, L, n, noverlap, nfft, *, nmels=0, nmfcc=0, twosided=0, elt=8, out_dev=1, sig_dev=1):
    return dump("bytes", kind, L, n, noverlap, nfft, nmels, nmfcc, twosided, elt, out_dev, sig_dev)["bytes"]


def pick(p, *keys):
    return tuple(p[k] for k in keys)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_frames_and_pairs_on_the_lds_path(dump):
    """L = 4096, n = 256, hop 64: (4096 - 256) / 64 + 1 = 61 frames in 31 pairs; 8192 / 256 = 32 pairs fit, the call has 31."""
    p = plan(dump, POWER, 4096, 256, 192, 256)
    assert pick(p, "hop", "frames", "pairs", "nbins", "rows", "nout") == (64, 61, 31, 129, 129, 61 * 129)
    assert pick(p, "path", "lds", "blue", "m", "len", "n1", "n2") == (1, 1, 0, 0, 256, 256, 1)
    assert pick(p, "pairs_per_workgroup", "fallback", "chunk_pairs", "slabs", "sum_chain", "refusal") == (31, 0, 0, 0, 0, OK)
    # n = 8: 1024 pairs fit the buffer, 512 is the cap, the call's 125 frames are 63 pairs
    p = plan(dump, POWER, 1000, 8, 0, 8)
    assert pick(p, "frames", "pairs", "pairs_per_workgroup", "path") == (125, 63, 63, 1)
    # ... and with frames to spare the cap holds: 512 pairs x 5 bins = 2560 split items <= 5120
    assert plan(dump, POWER, 8 * 4000, 8, 0, 8)["pairs_per_workgroup"] == 512
    # the split's registers: nfft = 64, 128 pairs x 33 bins = 4224 <= 5120; nfft = 16 with n = 10: 512 x 9 = 4608
    assert plan(dump, POWER, 64 * 4000, 64, 0, 64)["pairs_per_workgroup"] == 128
    assert plan(dump, POWER, 10 * 4000, 10, 0, 16)["pairs_per_workgroup"] == 512
    # a signal shorter than a frame: no frames, nothing sized
    p = plan(dump, POWER, 255, 256, 192, 256)
    assert pick(p, "frames", "pairs", "nout", "pairs_per_workgroup", "path", "refusal") == (0, 0, 0, 0, 1, OK)
    # rows by kind: bins, mel bands, coefficients; the frame average one- and two-sided
    assert plan(dump, MEL, 4096, 256, 192, 256, nmels=40)["rows"] == 40 and plan(dump, MFCC, 4096, 256, 192, 256, nmels=40, nmfcc=13)["rows"] == 13
    assert pick(plan(dump, WELCH, 4096, 256, 192, 256), "rows", "nout") == (129, 129)
    assert pick(plan(dump, WELCH, 4096, 256, 192, 256, twosided=1), "rows", "nout") == (256, 256)


def test_the_epilogue_regions_and_the_fallback(dump):
    """nfft = 8192: one pair fills the buffer.  mel with 40 bands: 2 (4097 + 40) = 8274 doubles per pair, 16384 / 8274 = 1 pair.  MFCC with
    4096 bands and 13 coefficients: 2 (4097 + 4096 + 13) = 16412 > 16384: no pair fits, the fallback."""
    p = plan(dump, MEL, 16384, 8192, 0, 8192, nmels=40)
    assert pick(p, "frames", "path", "pairs_per_workgroup", "fallback", "fallback_batch") == (2, 1, 1, 0, 0)
    p = plan(dump, MFCC, 16384, 8192, 0, 8192, nmels=4096, nmfcc=13)
    assert pick(p, "frames", "path", "pairs_per_workgroup", "fallback", "fallback_batch") == (2, 1, 0, 1, 1)
    # the fallback's own FFT launch: 8192 / 2048 = 4 pairs a workgroup (nfft = 2048, 2 (1025 + 8000 + 13) > 16384)
    p = plan(dump, MFCC, 2048 * 9, 2048, 0, 2048, nmels=8000, nmfcc=13)
    assert pick(p, "pairs_per_workgroup", "fallback", "fallback_batch") == (0, 1, 4)
    # mel at nfft = 256: 2 (129 + 40) = 338 doubles, 16384 / 338 = 48 > the buffer's 32
    assert plan(dump, MEL, 256 * 100, 256, 0, 256, nmels=40)["pairs_per_workgroup"] == 32
    # ... 2 (129 + 500) = 1258: 13 pairs
    assert plan(dump, MEL, 256 * 100, 256, 0, 256, nmels=500)["pairs_per_workgroup"] == 13


@pytest.mark.parametrize("nfft,m,n1,n2,path", [
    (4099, 8232, 84, 98, 4),           # 2 * 4099 - 1 = 8197 -> 8232 = 2^3 3 7^3
    (8191, 16384, 128, 128, 4),        # 16381 -> 2^14
    (16411, 32928, 168, 196, 4),       # 32821 -> 32928 = 2^5 3 7^3
    (11, 21, 21, 1, 3),                # 21 = 3 * 7, in LDS
    (4093, 8192, 8192, 1, 3),          # 8185 -> 2^13, the longest in LDS
])
def test_bluestein_lengths(dump, nfft, m, n1, n2, path):
    p = plan(dump, POWER, 3 * nfft, nfft, 0, nfft)
    assert pick(p, "blue", "m", "len", "n1", "n2", "path", "lds", "frames", "refusal") == (1, m, m, n1, n2, path, int(path == 3), 3, OK)


def test_four_step_chunks(dump):
    """A chunk's tmp + Z are 32 bytes per point and pair within 2^30 bytes: 2^30 / (32 * 16384) = 2048 pairs at nfft = 16384."""
    assert pick(plan(dump, POWER, 3 * 4099, 4099, 0, 4099), "pairs", "chunk_pairs", "pairs_per_workgroup") == (2, 2, 0)
    assert pick(plan(dump, POWER, 3 * 16384, 16384, 0, 16384), "path", "n1", "n2", "pairs", "chunk_pairs") == (2, 128, 128, 2, 2)
    assert plan(dump, POWER, 5000 * 16384, 16384, 0, 16384)["chunk_pairs"] == 2048
    assert plan(dump, MEL, 5000 * 16384, 16384, 0, 16384, nmels=40)["chunk_pairs"] == 2048
    # 2^30 / (32 * 8232) = 4076 pairs for the Bluestein length of 4099 (4076 * 263424 = 1073716224 <= 2^30 < 4077 of them)
    assert plan(dump, POWER, 10000 * 4099, 4099, 0, 4099)["chunk_pairs"] == 4076
    # one pair of nfft = 2^26 is 2^31 bytes: still a chunk of one
    assert pick(plan(dump, POWER, 3 * 2 ** 26, 2 ** 26, 0, 2 ** 26), "pairs", "chunk_pairs") == (2, 1)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n1,n2", [(16384, 128, 128), (73728, 256, 288), (33614, 98, 343), (4 * 10 ** 7, 6250, 6400), (2 ** 26, 8192, 8192)])
def test_splits(dump, N, n1, n2):
    assert dump("split", N) == dict(fits=1, len=N, n1=n1, n2=n2, smooth=1, radix_product=n1)


def test_what_has_no_split(dump):
    assert dump("split", 8192) == dict(fits=1, len=8192, n1=8192, n2=1, smooth=1, radix_product=8192)
    assert dump("split", 4099)["smooth"] == 0 and dump("split", 4099)["fits"] == 0
    assert dump("split", 2 ** 27) == dict(fits=0, len=0, n1=0, n2=0, smooth=1, radix_product=1)      # beyond 2^26
    # 7-smooth, within 2^26, but 3^16 = 43046721 = 6561^2: fits; 5 * 7^8 = 28824005 needs a factor 12005 or 16807 next to 2401 or 1715
    assert dump("split", 3 ** 16)["n1"] == 6561
    assert dump("split", 5 * 7 ** 8)["fits"] == 0


def test_refusals(dump):
    assert plan(dump, POWER, 2 ** 27, 1024, 0, 2 ** 26 + 1)["refusal"] == NFFT_TOO_LONG
    assert plan(dump, POWER, 2 ** 27, 1024, 0, 2 ** 26)["refusal"] == OK
    assert plan(dump, POWER, 2 ** 27, 1024, 0, 2 ** 26 - 1)["refusal"] == BLUESTEIN_TOO_LONG          # 2^27 - 3 < m means m > 2^26
    assert plan(dump, POWER, 2 ** 27, 1024, 0, 5 * 7 ** 8)["refusal"] == NO_SPLIT
    # the frame average at nfft = 8192: a pair a batch, 512 batches a slab: 2^40 + 1 frames of hop 1 are 2^39 + 1 pairs, 2^30 + 1 slabs
    n = 8192
    assert plan(dump, WELCH, n + 2 ** 40, n, n - 1, n)["refusal"] == TOO_MANY_SLABS
    assert pick(plan(dump, WELCH, n + 2 ** 40 - 1, n, n - 1, n), "refusal", "slabs", "slab_frames") == (OK, 2 ** 30, 1024)
    # ... and needs room for a pair on the LDS paths: it has it with nmels = 0, the only way it is called
    assert plan(dump, WELCH, 16384, 8192, 0, 8192)["refusal"] == OK
    assert plan(dump, WELCH, 16384, 8192, 0, 8192, nmels=4096)["refusal"] == WELCH_NO_PAIR


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n,noverlap,nfft,expected", [
    # 65533 frames in 32767 pairs, 32 a workgroup: 1024 batches, a slab each; F = 64, D = 63 + 10
    (2 ** 22, 256, 192, 256, dict(frames=65533, path=1, pairs_per_workgroup=32, batches=1024, slabs=1024, slab_frames=64, tree_depth=10, sum_chain=73)),
    # 40967 frames in 20484 pairs, 512 a workgroup: 41 batches of 1024 frames, the chain's cap: a slab each; D = 1023 + 6
    (40974, 8, 7, 8, dict(frames=40967, path=1, pairs_per_workgroup=512, batches=41, slabs=41, slab_frames=1024, tree_depth=6, sum_chain=1029)),
    # four-step: 2050 pairs in chunks of 2048: 4096 frames are 16 slabs, the last 4 frames one more; D = 255 + 5
    (4100 * 16384, 16384, 0, 16384, dict(frames=4100, path=2, chunk_pairs=2048, batches=0, slabs=17, slab_frames=256, tree_depth=5, sum_chain=260)),
    (5000, 5000, 0, 5000, dict(frames=1, path=1, pairs_per_workgroup=1, batches=1, slabs=1, slab_frames=1, tree_depth=0, sum_chain=0)),
    (3 * 8192, 8192, 0, 8192, dict(frames=3, path=1, pairs_per_workgroup=1, batches=2, slabs=2, slab_frames=2, tree_depth=1, sum_chain=2)),
    # the named cases of test_welch_host.py::test_chain_formula, asked of the header
    (2 ** 26, 2048, 1024, 2048, dict(frames=65535, path=1, pairs_per_workgroup=4, batches=8192, slabs=1024, slab_frames=64, sum_chain=73)),
    (2 ** 20, 2 ** 20, 0, 2 ** 20, dict(frames=1, path=2, chunk_pairs=1, slabs=1, sum_chain=0)),
    (2 * 8192, 8192, 0, 8192, dict(frames=2, path=1, pairs_per_workgroup=1, slabs=1, slab_frames=2, sum_chain=1)),
    # Bluestein, both families: 8 frames of 11 (m = 21) in one batch; 600 frames of 4099 (m = 8232) in one chunk, 3 slabs
    (88, 11, 0, 11, dict(frames=8, path=3, pairs_per_workgroup=4, batches=1, slabs=1, slab_frames=8, sum_chain=7)),
    (600 * 4099, 4099, 0, 4099, dict(frames=600, path=4, chunk_pairs=300, slabs=3, slab_frames=256, tree_depth=2, sum_chain=257)),
])
def test_frame_average(dump, L, n, noverlap, nfft, expected):
    p = plan(dump, WELCH, L, n, noverlap, nfft)
    assert {k: p[k] for k in expected} == expected and p["refusal"] == OK and p["fallback"] == 0


def test_more_batches_than_slabs(dump):
    """nfft = 256, 32 pairs a workgroup, 64 frames a batch: a workgroup may chain 1024 / 64 = 16 batches.  2^20 pairs are 32768 batches:
    more than 1024 x 16, so 2048 slabs of 16 batches, F = 1024, D = 1023 + 11."""
    p = plan(dump, WELCH, 2 ** 21 * 256, 256, 0, 256)
    assert pick(p, "frames", "batches", "slabs", "slab_frames", "sum_chain") == (2 ** 21, 32768, 2048, 1024, 1034)
    # 2049 batches on 1024 slabs: slab 0 holds batches 0, 1024 and 2048, the last of 2 frames only (131074 = 2048 * 64 + 2): F = 130
    p = plan(dump, WELCH, 131074 * 256, 256, 0, 256)
    assert pick(p, "batches", "slabs", "slab_frames", "sum_chain") == (2049, 1024, 130, 139)


def test_chain_bound_over_a_sweep(dump):
    """D <= 1100 wherever a workgroup's chain is capped at 1024 frames (the bound of test_welch_host.py::test_chain_formula, here on the
    header): LDS lengths 8192 / B with B = 1 .. 512 pairs a workgroup, four-step lengths 2^14 .. 2^26."""
    rng = np.random.default_rng(3)
    lds, four = [], []
    for _ in range(400):
        B = int(2 ** rng.integers(0, 10))
        K, n = int(rng.integers(1, 2 ** 26 // B + 2)), 8192 // B
        lds += [K * n, n, 0, n]
        flen = int(2 ** rng.integers(14, 27))
        four += [int(rng.integers(1, 100000)) * flen, flen, 0, flen]
    rows = dump("chains", *lds)
    assert len(rows) == 400
    for i, r in enumerate(rows):
        assert r["refusal"] == OK and r["path"] == 1 and r["frames"] == lds[4 * i] // lds[4 * i + 1], (i, r)
        assert 0 <= r["sum_chain"] <= 1023 + 26 and r["sum_chain"] <= 1100 and r["slabs"] >= 1, (i, r)
    rows = dump("chains", *four)
    assert len(rows) == 400
    for i, r in enumerate(rows):
        assert r["refusal"] == OK and r["path"] == 2 and r["pairs_per_workgroup"] == 0, (i, r)
        assert 0 <= r["sum_chain"] <= 255 + 17 and r["slabs"] >= 1, (i, r)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_device_bytes_of_the_staged_output_and_signal(dump):
    """Everything resident, the LDS path, power rows: nothing is allocated that the estimate counts."""
    a = (POWER, 4096, 256, 192, 256)
    assert nbytes(dump, *a) == 0
    assert nbytes(dump, *a, out_dev=0) == 8 * 61 * 129 == 62952            # 61 frames x 129 rows of doubles
    assert nbytes(dump, *a, out_dev=0, elt=4) == 31476
    assert nbytes(dump, *a, sig_dev=0) == 8 * 4096 == 32768
    assert nbytes(dump, *a, sig_dev=0, elt=4) == 16384
    assert nbytes(dump, *a, out_dev=0, sig_dev=0) == 62952 + 32768


def test_device_bytes_of_the_lds_paths(dump):
    """mel / MFCC count one pair's two power columns (16 bytes a bin) on every path; the fallback adds the frame flags and exponents, the
    power columns and the spectra of the whole call."""
    assert nbytes(dump, MEL, 16384, 8192, 0, 8192, nmels=40) == 16 * 4097 == 65552
    # 2 frames in 1 pair: 65552 + 2 * 4 * 2 + 8 * 2 * 4097 + 16 * 1 * 8192
    assert nbytes(dump, MFCC, 16384, 8192, 0, 8192, nmels=4096, nmfcc=13) == 65552 + 16 + 65552 + 131072 == 262192
    # 9 frames in 5 pairs of nfft = 2048: 16 * 1025 + 2 * 4 * 9 + 8 * 9 * 1025 + 16 * 5 * 2048
    assert nbytes(dump, MFCC, 2048 * 9, 2048, 0, 2048, nmels=8000, nmfcc=13) == 16400 + 72 + 73800 + 163840 == 254112


def test_device_bytes_of_the_four_step_paths(dump):
    """The minimum chunk is one pair: its spectrum and as much scratch (32 bytes a point), the flags and exponents of every frame; mel adds
    the pair's power columns."""
    assert nbytes(dump, POWER, 3 * 16384, 16384, 0, 16384) == 32 * 16384 + 2 * 4 * 3 == 524312
    assert nbytes(dump, MEL, 3 * 16384, 16384, 0, 16384, nmels=40) == 524312 + 16 * 8193 == 655400
    # ... and not the chunk the loop will take: 5000 frames count one pair and 5000 flags
    assert nbytes(dump, POWER, 5000 * 16384, 16384, 0, 16384) == 524288 + 40000 == 564288


def test_device_bytes_of_bluestein(dump):
    """Three vectors of m points (b, its transform, the four-step's scratch: counted on the LDS path too)."""
    assert nbytes(dump, POWER, 22, 11, 0, 11) == 3 * 16 * 21 == 1008
    # m = 8232, 3 frames: 3 * 16 * 8232 + 32 * 8232 + 2 * 4 * 3
    assert nbytes(dump, POWER, 3 * 4099, 4099, 0, 4099) == 395136 + 263424 + 24 == 658584


def test_device_bytes_of_the_frame_average(dump):
    """S slabs of nbins doubles; the output is one column."""
    assert nbytes(dump, WELCH, 2 ** 22, 256, 192, 256) == 8 * 1024 * 129 == 1056768
    assert nbytes(dump, WELCH, 2 ** 22, 256, 192, 256, out_dev=0) == 1056768 + 8 * 129
    assert nbytes(dump, WELCH, 2 ** 22, 256, 192, 256, out_dev=0, twosided=1) == 1056768 + 8 * 256
    assert nbytes(dump, WELCH, 2 ** 22, 256, 192, 256, sig_dev=0, elt=4) == 1056768 + 4 * 2 ** 22
    # four-step: 17 slabs of 8193 bins, one pair's spectrum and scratch, 4100 flags and exponents
    assert nbytes(dump, WELCH, 4100 * 16384, 16384, 0, 16384) == 8 * 17 * 8193 + 524288 + 32800 == 1671336
