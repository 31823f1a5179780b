"""What the batched-window engine decides on the host (csrc/windows_plan.h): the windows of a pass, the cut of a window
range into chunks and parts, the layout behind the packed inverses, fourier2complex.  The header has no HIP dependency: a tiny host
program is built against it and prints what it decides; CPU only.  Every expected value below is a literal worked from the rules, none
is computed by asking the header a second way.

    1  pass plan: cfg4's own shape and its variants, two passes, the dense form's cuts, the clamps, the segments
    2  chunk plan: cfg4, the shape and knob sets of test_chunked_engine_is_bit_identical_to_the_uncut_one, every way to the uncut engine,
       part ranges
    3  layout of the packed-inverse buffer, census to bytes
    4  fourier2complex"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: windows_plan_dump pass|chunk|parts|layout|census|f2c NUMBER ...  ->  one line of key=value pairs
PROGRAM = r"""
#include "windows_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<long long> v;
    for (int i = 2; i < argc; ++i) v.push_back(atoll(argv[i]));
    const auto need = [&](size_t k) { if (v.size() != k) exit(2); };
    if (!strcmp(argv[1], "pass")) {          // n Nf zerofreq ns nwin sparse init structured dense_rows budget_bytes
        need(10);
        const lpvs::WinPassPlan p = lpvs::window_pass_plan(v[0], v[1], v[2] != 0, v[3], v[4], v[5] != 0, v[6] != 0, v[7] != 0, v[8], (size_t)v[9]);
        printf("nreg=%lld np=%lld ld=%lld nmat=%d windows=%lld nrows=%lld panel_bytes=%zu seg_len=%lld segs=%d vb=%zu\n", (long long)p.nreg, (long long)p.np,
               (long long)p.ld, p.nmat, (long long)p.windows, (long long)p.nrows, p.panel_bytes, (long long)p.seg_len, p.segs, p.vb);
    } else if (!strcmp(argv[1], "chunk")) {  // nwin ns np iters sparse opt_chunk_mb opt_in_flight cache_bytes
        need(8);
        const lpvs::WinChunkPlan c = lpvs::window_chunk_plan(v[0], v[1], v[2], v[3], v[4] != 0, (int)v[5], (int)v[6], (double)v[7]);
        printf("chunked=%d chunk=%lld in_flight=%d applies=%d\n", (int)c.chunked, (long long)c.chunk, c.in_flight,
               (int)lpvs::window_chunking_applies(v[0], v[3], v[4] != 0, (int)v[5], (int)v[6]));
    } else if (!strcmp(argv[1], "parts")) {  // cw in_flight
        need(2);
        lpvs::WinChunkPlan c; c.in_flight = (int)v[1];
        const int parts = c.parts(v[0]);
        printf("parts=%d", parts);
        for (int p = 0; p < parts; ++p) printf(" lo%d=%lld hi%d=%lld", p, (long long)c.part_lo(v[0], parts, p), p, (long long)c.part_hi(v[0], parts, p));
        printf("\n");
    } else if (!strcmp(argv[1], "layout")) { // np elt nmat
        need(3);
        const lpvs::PackedLayout l = lpvs::packed_layout(v[0], (size_t)v[1], (size_t)v[2]);
        printf("tiles=%zu elems_bytes=%zu types_bytes=%zu absmax_off=%zu bytes=%zu\n", l.tiles, l.elems_bytes, l.types_bytes, l.absmax_off, l.bytes);
    } else if (!strcmp(argv[1], "census")) { // read32 format format ...
        if (v.empty()) return 2;
        std::vector<unsigned char> t(v.begin() + 1, v.end());
        const lpvs::TileCensus c = lpvs::tile_census(t.data(), t.size());
        printf("fixed=%zu diag=%zu total=%zu bytes=%.0f\n", c.fixed, c.diag, c.total, lpvs::census_stream_bytes(c, v[0] != 0));
    } else if (!strcmp(argv[1], "f2c")) {    // Nf zerofreq c0 c1 ...
        const long long Nf = v[0];
        std::vector<double> c(v.begin() + 2, v.end()), re((size_t)Nf, -1.0), im((size_t)Nf, -1.0);
        lpvs::fourier2complex(c.data(), Nf, v[1] != 0, re.data(), im.data());
        for (long long i = 0; i < Nf; ++i) printf("re%lld=%.0f im%lld=%.0f ", i, re[(size_t)i], i, im[(size_t)i]);
        printf("\n");
    } else return 2;
    return 0;
}
"""


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(mode, numbers...) -> the dict of integers the program prints."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("windows_plan")
    src, exe = os.path.join(d, "windows_plan_dump.cpp"), os.path.join(d, "windows_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(mode, *numbers):
        out = subprocess.check_output([exe, mode] + [str(int(x)) for x in numbers], text=True)
        return {k: int(v) for k, v in (kv.split("=") for kv in out.split())}
    yield run
    shutil.rmtree(d, ignore_errors=True)


GIB = 1 << 30
MIB = 1 << 20


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def pass_plan(dump, n, Nf, zerofreq, nwin, *, ns=1, sparse=1, init=0, structured=1, dense_rows=0, budget=48 * GIB):
    return dump("pass", n, Nf, zerofreq, ns, nwin, sparse, init, structured, dense_rows, budget)


def test_pass_plan_of_cfg4(dump):
    """n = 65536, 256 frequencies from zero: 511 regressors; two matrices of 2 MiB per window, 32 GiB hold 8192 of them."""
    assert pass_plan(dump, 65536, 256, 1, 1024) == dict(nreg=511, np=512, ld=512, nmat=2, windows=1024, nrows=65536, panel_bytes=0, seg_len=4096,
                                                         segs=16, vb=4194304)
    # ... before the cap by nwin: 2^35 / (8 * 512 * 512 * nmat)
    assert pass_plan(dump, 65536, 256, 1, 100000)["windows"] == 8192
    init = pass_plan(dump, 65536, 256, 1, 8192, init=1)
    assert (init["nmat"], init["windows"], init["vb"]) == (4, 4096, 16777216)
    assert pass_plan(dump, 65536, 256, 1, 1024, init=1)["windows"] == 1024
    dense = pass_plan(dump, 65536, 256, 1, 8192, sparse=0)
    assert (dense["nmat"], dense["windows"]) == (3, 5461)
    assert pass_plan(dump, 65536, 256, 1, 1024, sparse=0)["windows"] == 1024
    # two signals share the matrices: the windows of a pass do not change, the state vectors double
    assert pass_plan(dump, 65536, 256, 1, 1024, ns=2) == dict(nreg=511, np=512, ld=512, nmat=2, windows=1024, nrows=65536, panel_bytes=0, seg_len=4096,
                                                               segs=16, vb=8388608)


def test_pass_plan_takes_two_passes_at_2048_regressors(dump):
    """1024 frequencies without the zero frequency: two matrices of 32 MiB per window, 512 windows in 32 GiB."""
    assert pass_plan(dump, 65536, 1024, 0, 1024) == dict(nreg=2048, np=2048, ld=2048, nmat=2, windows=512, nrows=65536, panel_bytes=0, seg_len=4096,
                                                          segs=16, vb=8388608)
    assert pass_plan(dump, 65536, 1024, 1, 1024)["nreg"] == 2047


def test_pass_plan_of_the_dense_form(dump):
    """The panels: 48 GiB / (8 * 65536 * 512) = 192 windows at their nominal rows; the Gram plan may pad the rows, then fewer fit."""
    kw = dict(structured=0)
    assert pass_plan(dump, 65536, 256, 1, 1024, dense_rows=65536, **kw) == dict(nreg=511, np=512, ld=512, nmat=2, windows=192, nrows=65536,
                                                                                 panel_bytes=268435456, seg_len=0, segs=0, vb=786432)
    # 69632 rows: 285212672 bytes per window, 180 of them are 51338280960 <= 48 GiB = 51539607552 < 181 of them
    padded = pass_plan(dump, 65536, 256, 1, 1024, dense_rows=69632, **kw)
    assert (padded["windows"], padded["panel_bytes"], padded["nrows"]) == (180, 285212672, 69632)
    # the matrices do not bound a dense-form pass: the dense estimator and init = true change nmat only
    assert pass_plan(dump, 65536, 256, 1, 1024, dense_rows=65536, sparse=0, **kw)["windows"] == 192
    assert pass_plan(dump, 65536, 256, 1, 1024, dense_rows=65536, init=1, **kw)["windows"] == 192
    # the shape of the second-pass test (tests/test_gpu_windows.py): 8 MiB per window, 128 in 1 GiB, 140 in the default budget
    assert pass_plan(dump, 4096, 100, 0, 140, ns=2, dense_rows=4096, budget=GIB, **kw) == dict(nreg=200, np=256, ld=256, nmat=2, windows=128, nrows=4096,
                                                                                                panel_bytes=8388608, seg_len=0, segs=0, vb=524288)
    assert pass_plan(dump, 4096, 100, 0, 140, dense_rows=4608, budget=GIB, **kw)["windows"] == 113      # 1 GiB / 9437184
    assert pass_plan(dump, 4096, 100, 0, 140, dense_rows=4096, **kw)["windows"] == 140
    # n is rounded up to 64 at the first cut: 1 GiB / (8 * 4032 * 256) = 130, and the true rows (4000) leave it there
    assert pass_plan(dump, 4000, 100, 0, 1000, dense_rows=4000, budget=GIB, **kw)["windows"] == 130


def test_pass_plan_clamps(dump):
    # at 1: a budget below one window's panels, before and after the true rows
    assert pass_plan(dump, 65536, 256, 1, 1024, structured=0, dense_rows=65536, budget=MIB)["windows"] == 1
    assert pass_plan(dump, 64, 256, 1, 1024, structured=0, dense_rows=65536, budget=128 * MIB)["windows"] == 1     # first cut 512, one true panel 256 MiB
    # at 1: structured, four matrices of 8 GiB each (np = 32768) are the whole 32 GiB
    assert pass_plan(dump, 65536, 16384, 0, 1024, init=1)["windows"] == 1
    assert pass_plan(dump, 65536, 16384, 0, 1024)["windows"] == 2
    # at nwin
    assert pass_plan(dump, 65536, 256, 1, 5)["windows"] == 5
    assert pass_plan(dump, 65536, 256, 1, 1)["windows"] == 1
    assert pass_plan(dump, 65536, 256, 1, 100, structured=0, dense_rows=65536)["windows"] == 100
    # at 8192: 64 regressors, 2^35 / (8 * 128 * 128 * 2) = 131072 windows' matrices; 48 GiB / (8 * 64 * 256) = 393216 windows' panels
    small = pass_plan(dump, 64, 32, 0, 100000)
    assert (small["nreg"], small["np"], small["ld"], small["windows"]) == (64, 128, 256, 8192)
    assert pass_plan(dump, 64, 32, 0, 100000, structured=0, dense_rows=64)["windows"] == 8192
    assert pass_plan(dump, 64, 32, 0, 8191)["windows"] == 8191


@pytest.mark.parametrize("n,seg_len,segs", [(1000, 1000, 1), (4095, 4095, 1), (4096, 4096, 1), (4097, 4096, 2), (10000, 4096, 3), (65536, 4096, 16)])
def test_pass_plan_segments(dump, n, seg_len, segs):
    p = pass_plan(dump, n, 256, 1, 8)
    assert (p["seg_len"], p["segs"], p["nrows"]) == (seg_len, segs, n)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
CACHE = 256 * MIB
UNCUT = -1                                            # LPVS_WINDOW_UNCUT (include/lpvspectral.h); what LPVS_WINDOW_CHUNK_MB=0 becomes


def chunk_plan(dump, nwin, np_, *, ns=1, iters=2000, sparse=1, chunk_mb=0, in_flight=0, cache=CACHE):
    p = dump("chunk", nwin, ns, np_, iters, sparse, chunk_mb, in_flight, cache)
    assert p.pop("applies") == p["chunked"]
    return p


def parts(dump, cw, in_flight):
    p = dump("parts", cw, in_flight)
    return [(p[f"lo{i}"], p[f"hi{i}"]) for i in range(p["parts"])]


def test_chunk_plan_of_cfg4(dump):
    """np = 512: ten tiles of 74240 bytes, 742400 per window; 1.0625 * 256 MiB = 285212672 bytes hold 384 windows; 1024 windows are three
    chunks, evened to 342, 342, 340, each in halves."""
    assert dump("layout", 512, 6, 1)["tiles"] == 10
    assert dump("census", 0, 1) == dict(fixed=1, diag=0, total=1, bytes=74240)
    assert chunk_plan(dump, 1024, 512) == dict(chunked=1, chunk=342, in_flight=2)
    assert parts(dump, 342, 2) == [(0, 171), (171, 342)] and parts(dump, 340, 2) == [(0, 170), (170, 340)]
    # the first cut itself: 384 windows are one chunk, 385 are two of 193
    assert chunk_plan(dump, 384, 512)["chunk"] == 384 and chunk_plan(dump, 385, 512)["chunk"] == 193
    # two signals: twice the weight per window, 192 at the first cut -> six chunks of 171
    assert chunk_plan(dump, 1024, 512, ns=2)["chunk"] == 171
    # another cache: 128 MiB hold 192 windows
    assert chunk_plan(dump, 1024, 512, cache=128 * MIB)["chunk"] == 171
    # an explicit size in MB (decimal): 100 MB / 742400 = 134 windows -> eight chunks of 128
    assert chunk_plan(dump, 1024, 512, chunk_mb=100)["chunk"] == 128


@pytest.mark.parametrize("knobs,ns,chunk,in_flight,first_parts,last_cw,last_parts", [
    # 192 regressors, np = 256: three tiles, 222720 bytes per window and signal
    ((3, 2), 1, 14, 2, [(0, 14)], 13, [(0, 13)]),                     # 3 MB: 13 windows, raised to 16 -> six chunks, evened to 14; too short to halve
    ((3, 2), 2, 14, 2, [(0, 14)], 13, [(0, 13)]),                     # (6 windows, raised to 16)
    ((UNCUT, 3), 1, 83, 3, [(0, 27), (27, 55), (55, 83)], 83, [(0, 27), (27, 55), (55, 83)]),
    ((UNCUT, 3), 2, 83, 3, [(0, 27), (27, 55), (55, 83)], 83, [(0, 27), (27, 55), (55, 83)]),
    ((5, 1), 1, 21, 1, [(0, 21)], 20, [(0, 20)]),                     # 5 MB: 22 windows -> four chunks, evened to 21
    ((5, 1), 2, 14, 1, [(0, 14)], 13, [(0, 13)]),                     # 11 windows, raised to 16
    ((0, 0), 1, 83, 2, [(0, 41), (41, 83)], 83, [(0, 41), (41, 83)]),  # the defaults: 285 MB hold every window, two parts
    ((0, 0), 2, 83, 2, [(0, 41), (41, 83)], 83, [(0, 41), (41, 83)]),
])
def test_chunk_plan_of_the_chunked_engine_test(dump, knobs, ns, chunk, in_flight, first_parts, last_cw, last_parts):
    """83 windows of np = 256 under the four knob sets of test_chunked_engine_is_bit_identical_to_the_uncut_one, on one signal (psd) and two (csd)."""
    assert chunk_plan(dump, 83, 256, ns=ns, iters=150, chunk_mb=knobs[0], in_flight=knobs[1]) == dict(chunked=1, chunk=chunk, in_flight=in_flight)
    assert parts(dump, chunk, in_flight) == first_parts
    assert last_cw == 83 - (-(-83 // chunk) - 1) * chunk                                   # the ragged last chunk
    assert parts(dump, last_cw, in_flight) == last_parts


def test_what_goes_to_the_uncut_engine(dump):
    uncut = dict(chunked=0, chunk=0)
    for kw in (dict(sparse=0), dict(iters=63), dict(chunk_mb=UNCUT, in_flight=1)):
        p = chunk_plan(dump, 1024, 512, **kw)
        assert {k: p[k] for k in uncut} == uncut, kw
    assert chunk_plan(dump, 15, 512)["chunked"] == 0
    # ... and their neighbours that do not
    assert chunk_plan(dump, 16, 512) == dict(chunked=1, chunk=16, in_flight=2)
    assert chunk_plan(dump, 1024, 512, iters=64)["chunked"] == 1
    assert chunk_plan(dump, 1024, 512, chunk_mb=UNCUT) == dict(chunked=1, chunk=1024, in_flight=2)              # one chunk in halves
    assert chunk_plan(dump, 1024, 512, chunk_mb=UNCUT, in_flight=2) == dict(chunked=1, chunk=1024, in_flight=2)
    assert chunk_plan(dump, 1024, 512, in_flight=1) == dict(chunked=1, chunk=342, in_flight=1)                  # chunks, one part each
    assert chunk_plan(dump, 1024, 512, chunk_mb=1, in_flight=1) == dict(chunked=1, chunk=16, in_flight=1)       # (1 window, raised to 16)


@pytest.mark.parametrize("cw,in_flight,expected", [
    (342, 1, [(0, 342)]), (31, 2, [(0, 31)]), (32, 2, [(0, 16), (16, 32)]), (33, 2, [(0, 16), (16, 33)]),
    (47, 3, [(0, 47)]), (48, 3, [(0, 16), (16, 32), (32, 48)]), (50, 3, [(0, 16), (16, 33), (33, 50)]), (340, 3, [(0, 113), (113, 226), (226, 340)]),
    (64, 4, [(0, 16), (16, 32), (32, 48), (48, 64)]), (63, 4, [(0, 63)])])
def test_parts_tile_a_chunk(dump, cw, in_flight, expected):
    got = parts(dump, cw, in_flight)
    assert got == expected
    assert got[0][0] == 0 and got[-1][1] == cw and all(a[1] == b[0] for a, b in zip(got, got[1:])) and all(lo < hi for lo, hi in got)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_,nmat,expected", [
    (256, 1, dict(tiles=3, elems_bytes=294912, types_bytes=256, absmax_off=295168, bytes=295424)),
    (256, 1024, dict(tiles=3, elems_bytes=301989888, types_bytes=3072, absmax_off=301992960, bytes=302001152)),
    (512, 1, dict(tiles=10, elems_bytes=983040, types_bytes=256, absmax_off=983296, bytes=983552)),
    (512, 1024, dict(tiles=10, elems_bytes=1006632960, types_bytes=10240, absmax_off=1006643200, bytes=1006651392)),
    (32768, 1, dict(tiles=32896, elems_bytes=3233808384, types_bytes=33024, absmax_off=3233841408, bytes=3233841664)),
    (32768, 1024, dict(tiles=32896, elems_bytes=3311419785216, types_bytes=33685504, absmax_off=3311453470720, bytes=3311453478912)),
])
def test_layout_of_the_packed_inverses(dump, np_, nmat, expected):
    """6-byte elements, one format byte per tile rounded up to 256, then 8 bytes of max|M| per matrix (256 at least: a single matrix leaves
    its largest row sum beside it)."""
    assert dump("layout", np_, 6, nmat) == expected


def test_layout_of_the_other_element_sizes(dump):
    assert dump("layout", 512, 8, 1)["elems_bytes"] == 1310720 and dump("layout", 512, 4, 1)["elems_bytes"] == 655360
    assert dump("layout", 512, 8, 1024)["elems_bytes"] == 1342177280                       # what the engine allocates for 1024 windows
    assert dump("layout", 512, 6, 1024)["bytes"] < 1342177280                              # ... and the 6-byte layout with its tail fits it
    assert dump("layout", 512, 6, 3) == dict(tiles=10, elems_bytes=2949120, types_bytes=256, absmax_off=2949376, bytes=2949632)
    assert dump("layout", 512, 6, 40)["bytes"] == 39321600 + 512 + 320                     # (400 format bytes -> 512; 8 * 40 > 256)


def test_census_to_bytes(dump):
    """Per tile: 74240 (36-bit fixed point), 66048 (its 32-bit reads), 98304 (float head + tail); 1024 more for a fixed-point diagonal tile."""
    all_fixed, with_diag, all_float = [1] * 10, [2, 1, 2, 1, 1, 2, 1, 1, 1, 2], [0] * 10
    mixed = [0, 1, 0, 1, 1, 0, 1, 1, 1, 0]
    assert dump("census", 0, *all_fixed) == dict(fixed=10, diag=0, total=10, bytes=742400)
    assert dump("census", 1, *all_fixed) == dict(fixed=10, diag=0, total=10, bytes=660480)
    assert dump("census", 0, *with_diag) == dict(fixed=10, diag=4, total=10, bytes=746496)
    assert dump("census", 1, *with_diag) == dict(fixed=10, diag=4, total=10, bytes=664576)
    assert dump("census", 0, *all_float) == dump("census", 1, *all_float) == dict(fixed=0, diag=0, total=10, bytes=983040)
    assert dump("census", 0, *mixed) == dict(fixed=6, diag=0, total=10, bytes=838656)
    assert dump("census", 1, *mixed) == dict(fixed=6, diag=0, total=10, bytes=789504)
    assert dump("census", 0, 2, 0, 1) == dict(fixed=2, diag=1, total=3, bytes=247808)       # 2 * 74240 + 1024 + 98304


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_fourier2complex(dump):
    """src/utilities.jl:62-73: [cos; sin] -> cos + i sin; with the zero frequency there is no first sine, and its imaginary part is 0."""
    assert dump("f2c", 3, 0, 1, 2, 3, 4, 5, 6) == dict(re0=1, im0=4, re1=2, im1=5, re2=3, im2=6)
    assert dump("f2c", 3, 1, 1, 2, 3, 4, 5) == dict(re0=1, im0=0, re1=2, im1=4, re2=3, im2=5)
    assert dump("f2c", 1, 1, 7) == dict(re0=7, im0=0)
