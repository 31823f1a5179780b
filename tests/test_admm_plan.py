"""What the ADMM handle decides on the host (csrc/admm_plan.h): the correction schedule, the storage of the packed inverse,
which iteration runs, how a run is cut.  The header has no HIP dependency: a tiny host program is built against it and prints what it
decides; CPU only.  Every expected value below is a literal worked from the rules, none is computed by asking the header a second way.

    1  correction points of the default schedules and of every LPVS_XUPDATE_CORRECTION experiment string
    2  run cuts: chunked calls against one call, the steps of a 2000-iteration run, graph replays
    3  refreshes of the stale nibble product: the counts the GPU tests assert on the device, the count the comment at NibKnobs states
    4  storage plan, repacking, demotion, the knob parsers
    5  iteration kind: one row per clause of each predicate
    6  closure: every IterationKind and every storage mode occurs in the tables"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: admm_plan_dump MODE ARGUMENT ...  ->  one line of key=value pairs (a value is an integer or a comma-separated list of integers)
PROGRAM = r"""
#include "admm_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
using namespace lpvs;
static void list(const char *key, const std::vector<long long> &v) {
    printf("%s=", key);
    for (size_t i = 0; i < v.size(); ++i) printf(i ? ",%lld" : "%lld", v[i]);
    printf(" ");
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    std::vector<long long> v;
    for (int i = 2; i < argc; ++i) v.push_back(atoll(argv[i]));
    const auto need = [&](size_t k) { if (v.size() != k) exit(2); };
    if (mode == "cuts") {                 // SPEC ("-": no experiment string) ns corrected k0 chunk ...: lpvs_admm_run's loop, call by call
        if (v.size() < 5) return 2;
        const XcorrSchedule s = xcorr_schedule_from(strcmp(argv[2], "-") ? argv[2] : nullptr, xcorr_default_schedule(v[1], v[2] != 0));
        long long k = v[3];
        std::vector<long long> steps, corrections;
        for (size_t c = 4; c < v.size(); ++c)
            for (long long todo = v[c]; todo > 0;) {
                const RunStep r = next_run_step(s, k, todo);
                if (r.step <= 0 || r.step > todo) return 3;
                steps.push_back(r.step); k += r.step; todo -= r.step;
                if (r.correct_after) corrections.push_back(k);
            }
        printf("on=%d ", (int)s.on()); list("steps", steps); list("corrections", corrections); printf("\n");
    } else if (mode == "replays") {       // np todo chunk graphs_allowed
        need(4);
        const long long r = graph_replays(v[0], v[1], v[2], v[3] != 0);
        printf("replays=%lld left=%lld\n", r, v[1] - r * v[2]);
    } else if (mode == "chunk_iters") {   // IterationKind
        need(1);
        printf("iters=%lld\n", (long long)graph_chunk_iters((IterationKind)v[0]));
    } else if (mode == "nib") {           // g0 g1 period ramp
        need(4);
        std::vector<long long> due;
        for (long long g = v[0]; g < v[1] && due.size() < 64; ++g) if (nib_refresh_due(g, (int)v[2], (int)v[3])) due.push_back(g);
        printf("count=%lld ", nib_refreshes_between(v[0], v[1], (int)v[2], (int)v[3])); list("first_due", due); printf("\n");
    } else if (mode == "storage" || mode == "demoted") {   // np ns f32 storage_option multi_fixed_ok corrected fix_bits period ramp
        need(9);
        NibKnobs nib; nib.period = (int)v[7]; nib.ramp = (int)v[8];
        StoragePlan p = admm_storage_plan(v[0], v[1], v[2] != 0, (int)v[3], v[4] != 0, v[5] != 0, (int)v[6], nib);
        if (mode == "demoted") p = demoted_plan(p);
        printf("mode=%d read32=%d fix_bits=%d nib_period=%d nib_ramp=%d element_bytes=%zu bytes=%zu diag_float=%d want_rowsum=%d offset_form=%d owns_fi=%d\n",
               p.mode, (int)p.read32, p.fix_bits, p.nib_period, p.nib_ramp, p.element_bytes, p.bytes, (int)p.diag_float, (int)p.want_rowsum,
               (int)p.offset_form, (int)p.owns_fi);
    } else if (mode == "repack") {        // valid have_mode have_fix_bits have_demoted want_mode want_fix_bits
        need(6);
        printf("repack=%d\n", (int)must_repack(v[0] != 0, (int)v[1], (int)v[2], v[3] != 0, (int)v[4], (int)v[5]));
    } else if (mode == "demote") {        // fixed tiles
        need(2);
        printf("demote=%d\n", (int)demote_to_split((size_t)v[0], (size_t)v[1]));
    } else if (mode == "knobs") {         // NAME=VALUE ...
        std::map<std::string, std::string> env;
        for (int i = 2; i < argc; ++i) { const std::string a = argv[i]; env[a.substr(0, a.find('='))] = a.substr(a.find('=') + 1); }
        const auto get = [&](const char *name) -> const char * { const auto it = env.find(name); return it == env.end() ? nullptr : it->second.c_str(); };
        const NibKnobs k = nib_knobs_from(get);
        printf("period=%d ramp=%d fix_bits=%d\n", k.period, k.ramp, fix_bits_from(get));
    } else if (mode == "iter") {          // np n ns prox group_len two packed partials offset formats split f32 fi ctl scratch nrhs nbatch
        need(17);
        IterFacts f;
        f.np = v[0]; f.n = v[1]; f.ns = (int)v[2]; f.prox_kind = (int)v[3]; f.group_len = v[4]; f.option_two = v[5] != 0;
        f.packed = v[6] != 0; f.partials = v[7] != 0; f.offset = v[8] != 0; f.tile_formats = v[9] != 0; f.split_copy = v[10] != 0; f.f32_copy = v[11] != 0;
        f.fi = v[12] != 0; f.small_ctl = v[13] != 0; f.scratch = v[14] != 0; f.nrhs = (int)v[15]; f.nbatch = v[16];
        printf("fusable=%d one=%d small=%d batch=%d kind=%d\n", (int)prox_fusable(f), (int)one_launch_applies(f), (int)small_one_launch_applies(f),
               (int)batch_one_launch_applies(f), (int)iteration_kind(f));
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
    """dump(mode, arguments...) -> the dict the program prints: integers, and lists of integers for the keys that hold lists."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("admm_plan")
    src, exe = os.path.join(d, "admm_plan_dump.cpp"), os.path.join(d, "admm_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)
    lists = ("steps", "corrections", "first_due")

    def run(mode, *args):
        out = subprocess.check_output([exe, mode] + [str(a) for a in args], text=True)
        kv = dict(item.split("=") for item in out.split())
        return {k: ([int(x) for x in v.split(",") if x] if k in lists else int(v)) for k, v in kv.items()}
    yield run
    shutil.rmtree(d, ignore_errors=True)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def corrections(dump, spec, *, ns=1, corrected=1, chunks=(2099,), k0=0):
    """Iterations after which a correction is scheduled when `chunks` are run call by call ((2099,): every point in [0, 2100))."""
    return dump("cuts", spec, ns, corrected, k0, *chunks)["corrections"]


ONE_RHS = [16, 128, 256, 512, 1024, 2048]
SEVERAL_RHS = [16, 512, 1024, 2048]


def test_default_correction_points(dump):
    assert corrections(dump, "-") == ONE_RHS
    assert corrections(dump, "-", ns=2) == SEVERAL_RHS and corrections(dump, "-", ns=8) == SEVERAL_RHS
    off = dump("cuts", "-", 1, 0, 0, 2099)
    assert off == dict(on=0, steps=[2099], corrections=[])
    assert dump("cuts", "3", 1, 0, 0, 2099)["on"] == 1       # (the handle hands the string over only when the correction is on)


@pytest.mark.parametrize("spec,points", [
    ("3", [1, 3, 9, 27, 81, 243, 729]),
    ("2", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048]),
    ("e100", [16] + list(range(100, 2100, 100))),
    ("e8", list(range(8, 2100, 8))),                         # (no extra 16)
    ("e16", list(range(16, 2100, 16))),
    ("d64", [16, 64, 128, 256, 512, 1024, 2048]),
    ("d8", [8, 16, 32, 64, 128, 256, 512, 1024, 2048]),
    ("q128", [1, 2, 4, 8, 16, 128, 256, 512, 1024, 2048]),
])
def test_correction_points_of_the_schedule_experiments(dump, spec, points):
    assert corrections(dump, spec) == points
    assert corrections(dump, spec, ns=2) == points           # an explicit schedule does not look at the right-hand sides


@pytest.mark.parametrize("spec", ["0", "1", "on", "e0", "x", "1x", "true", "d", "q-4", "e", ""])
def test_anything_else_keeps_the_default_schedule(dump, spec):
    """"1" once fell through to silently off."""
    assert corrections(dump, spec) == ONE_RHS
    assert corrections(dump, spec, ns=2) == SEVERAL_RHS


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_the_correction_points_do_not_depend_on_the_chunking(dump):
    """The chunking of test_correction_schedule_is_absolute_and_the_offset_is_state: the first three points fall on chunk ends."""
    whole = dump("cuts", "-", 1, 1, 0, 600)
    assert whole == dict(on=1, steps=[16, 112, 128, 256, 88], corrections=[16, 128, 256, 512])
    chunked = dump("cuts", "-", 1, 1, 0, 10, 6, 1, 110, 1, 127, 1, 200, 144)
    assert chunked == dict(on=1, steps=[10, 6, 1, 110, 1, 127, 1, 200, 56, 88], corrections=[16, 128, 256, 512])


def test_the_steps_of_a_2000_iteration_run(dump):
    assert dump("cuts", "-", 1, 1, 0, 2000) == dict(on=1, steps=[16, 112, 128, 256, 512, 976], corrections=[16, 128, 256, 512, 1024])
    assert dump("cuts", "-", 8, 1, 0, 2000) == dict(on=1, steps=[16, 496, 512, 976], corrections=[16, 512, 1024])
    assert dump("cuts", "-", 1, 0, 0, 2000) == dict(on=0, steps=[2000], corrections=[])
    # re-entry at 40 (lpvs_admm_set_state): the schedule is absolute
    assert dump("cuts", "-", 1, 1, 40, 100) == dict(on=1, steps=[88, 12], corrections=[128])


def test_a_call_shorter_than_the_distance_to_the_next_correction(dump):
    assert dump("cuts", "-", 1, 1, 20, 50) == dict(on=1, steps=[50], corrections=[])
    assert dump("cuts", "-", 1, 1, 20, 107) == dict(on=1, steps=[107], corrections=[])
    assert dump("cuts", "-", 1, 1, 20, 108) == dict(on=1, steps=[108], corrections=[128])   # ends on it: corrected, nothing left
    assert dump("cuts", "-", 1, 1, 20, 109) == dict(on=1, steps=[108, 1], corrections=[128])


TWO_LAUNCH, ONE_LAUNCH, SMALL_ONE_LAUNCH, BATCH_ONE_LAUNCH = 0, 1, 2, 3      # enum class IterationKind


def test_graph_replays(dump):
    """A captured chunk is replayed while at least two chunks remain, below np = 2048 only."""
    assert dump("chunk_iters", SMALL_ONE_LAUNCH)["iters"] == 250
    assert [dump("chunk_iters", k)["iters"] for k in (TWO_LAUNCH, ONE_LAUNCH, BATCH_ONE_LAUNCH)] == [50, 50, 50]
    assert dump("replays", 1024, 499, 250, 1) == dict(replays=0, left=499)
    assert dump("replays", 1024, 500, 250, 1) == dict(replays=2, left=0)
    assert dump("replays", 1024, 749, 250, 1) == dict(replays=2, left=249)
    assert dump("replays", 1024, 600, 250, 1) == dict(replays=2, left=100)
    assert dump("replays", 1024, 99, 50, 1) == dict(replays=0, left=99)
    assert dump("replays", 1024, 100, 50, 1) == dict(replays=2, left=0)
    assert dump("replays", 1024, 2000, 50, 1) == dict(replays=40, left=0)
    assert dump("replays", 1024, 2000, 250, 0) == dict(replays=0, left=2000)     # LPVS_NO_GRAPH
    assert dump("replays", 2048, 2000, 250, 1) == dict(replays=0, left=2000)
    assert dump("replays", 1920, 2000, 250, 1) == dict(replays=8, left=0)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_nibble_refreshes_of_the_default_knobs(dump):
    """Period 32, ramp 8: after every launch up to 15, every 2nd up to 31, 4th up to 63, 8th up to 127, 16th up to 255, then every 32nd."""
    first = list(range(16)) + list(range(16, 32, 2)) + list(range(32, 64, 4)) + [64]
    assert dump("nib", 0, 70, 32, 8) == dict(count=33, first_due=first)                        # 16 + 8 + 8 + 1: test_gpu_xupdate_correction.py
    assert dump("nib", 0, 90, 32, 8)["count"] == 36                                             # ... + 72, 80, 88
    assert dump("nib", 0, 2000, 32, 8)["count"] == 103                                          # 16 + 8 + 8 + 8 + 8 + 55 (256 .. 1984): the comment at NibKnobs
    # from inside an octave: 104, 112, 120; eight multiples of 16 from 128; 256 and 288
    assert dump("nib", 100, 300, 32, 8) == dict(count=13, first_due=[104, 112, 120, 128, 144, 160, 176, 192, 208, 224, 240, 256, 288])


def test_nibble_refreshes_without_a_ramp(dump):
    assert dump("nib", 0, 100, 32, 0) == dict(count=5, first_due=[0, 1, 32, 64, 96])
    assert dump("nib", 1, 100, 32, 0) == dict(count=4, first_due=[1, 32, 64, 96])
    assert dump("nib", 2, 100, 32, 0) == dict(count=3, first_due=[32, 64, 96])
    assert dump("nib", 0, 5, 1, 0) == dict(count=5, first_due=[0, 1, 2, 3, 4])                  # (g = 1 is not counted twice)
    assert dump("nib", 0, 100, 0, 8) == dict(count=0, first_due=[])                             # period 0: the 36-bit reads
    # period 4, ramp 1: the step is min(4, 2^floor(log2 g)) -- 1 up to g = 1, 2 up to 3, then 4
    assert dump("nib", 0, 40, 4, 1) == dict(count=12, first_due=[0, 1, 2, 4, 8, 12, 16, 20, 24, 28, 32, 36])


@pytest.mark.parametrize("cuts", [(0, 70), (0, 1, 70), (0, 16, 17, 33, 64, 65, 70), (0, 10, 16, 17, 127, 128, 255, 256, 456, 512, 600), tuple(range(0, 71))])
def test_any_split_of_a_range_sums_to_the_whole(dump, cuts):
    whole = {70: 33, 600: 59}[cuts[-1]]                      # [0, 600): 16 + 8 + 8 + 8 + 8 + 11 (256 .. 576)
    assert sum(dump("nib", a, b, 32, 8)["count"] for a, b in zip(cuts, cuts[1:])) == whole


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
NONE, F64, F32, SPLIT, MIXED = 0, 1, 2, 3, 4                  # kMp*
O_DEFAULT, O_MIXED, O_SPLIT, O_F64, O_MIXED32 = 0, 1, 2, 3, 4  # LPVS_STORAGE_* (include/lpvspectral.h)

# np = 2048: 16 row blocks, 136 tiles of 16384 elements; 49152: 384 blocks, 73920 tiles; 49280: 385 blocks, 74305 tiles.
# Mixed adds one format byte per tile rounded up to 256 (256 / 73984 / 74496) and 256 bytes for max|M| and the row sum.
STORAGE_ROWS = [
    # np, ns, f32, option, multi_fixed_ok, corrected  ->  mode, read32, element bytes, bytes, diag_float, want_rowsum, owns_fi
    ((1920, 1, 0, O_DEFAULT, 1, 0), (NONE, 0, 0, 0, 0, 0, 0)),
    ((1920, 1, 0, O_DEFAULT, 1, 1), (NONE, 0, 0, 0, 0, 0, 0)),           # (no handle below 2048 is corrected; nothing to read 32 bits of)
    ((1920, 2, 0, O_F64, 1, 0), (NONE, 0, 0, 0, 0, 0, 0)),
    ((1920, 1, 1, O_DEFAULT, 1, 0), (NONE, 0, 0, 0, 0, 0, 0)),
    ((2048, 1, 0, O_DEFAULT, 1, 1), (MIXED, 1, 6, 13369856, 0, 1, 1)),
    ((2048, 1, 0, O_DEFAULT, 0, 1), (MIXED, 1, 6, 13369856, 0, 1, 1)),   # (multi_fixed_ok speaks of several right-hand sides only)
    ((2048, 1, 0, O_DEFAULT, 1, 0), (MIXED, 0, 6, 13369856, 0, 1, 1)),   # correction off: the 36-bit reads
    ((2048, 1, 0, O_MIXED, 1, 1), (MIXED, 0, 6, 13369856, 0, 1, 1)),     # MIXED by name asks for the 36-bit reads
    ((2048, 1, 0, O_MIXED32, 1, 1), (MIXED, 1, 6, 13369856, 0, 1, 1)),
    ((2048, 1, 0, O_MIXED32, 1, 0), (MIXED, 0, 6, 13369856, 0, 1, 1)),
    ((2048, 1, 0, O_SPLIT, 1, 1), (SPLIT, 0, 6, 13369344, 0, 0, 0)),
    ((2048, 1, 0, O_F64, 1, 1), (F64, 0, 8, 17825792, 0, 0, 0)),
    ((2048, 1, 1, O_DEFAULT, 1, 1), (F32, 0, 4, 8912896, 0, 0, 1)),      # f32 never reads 32-bit fixed point
    ((2048, 1, 1, O_MIXED32, 1, 1), (F32, 0, 4, 8912896, 0, 0, 1)),
    ((2048, 1, 1, O_F64, 1, 1), (F32, 0, 4, 8912896, 0, 0, 1)),          # ... and streams floats whatever the option says
    ((2048, 1, 1, O_SPLIT, 1, 0), (F32, 0, 4, 8912896, 0, 0, 1)),
    ((2048, 2, 0, O_DEFAULT, 1, 1), (MIXED, 0, 6, 13369856, 1, 0, 0)),   # several right-hand sides: diagonal tiles float-head, 36-bit reads
    ((2048, 2, 0, O_MIXED32, 1, 1), (MIXED, 0, 6, 13369856, 1, 0, 0)),
    ((2048, 2, 0, O_DEFAULT, 0, 1), (SPLIT, 0, 6, 13369344, 0, 0, 0)),   # the tile product in use does not read fixed-point tiles
    ((2048, 2, 0, O_MIXED, 0, 0), (SPLIT, 0, 6, 13369344, 0, 0, 0)),
    ((2048, 2, 0, O_SPLIT, 1, 1), (SPLIT, 0, 6, 13369344, 0, 0, 0)),
    ((2048, 2, 0, O_F64, 1, 1), (F64, 0, 8, 17825792, 0, 0, 0)),
    ((2048, 2, 1, O_DEFAULT, 1, 1), (F32, 0, 4, 8912896, 0, 0, 0)),      # (one-launch records: one right-hand side only)
    ((49152, 2, 0, O_DEFAULT, 1, 1), (MIXED, 0, 6, 7266705920, 1, 0, 0)),
    ((49152, 2, 0, O_SPLIT, 1, 1), (SPLIT, 0, 6, 7266631680, 0, 0, 0)),
    ((49152, 2, 0, O_F64, 1, 0), (F64, 0, 8, 9688842240, 0, 0, 0)),
    ((49152, 1, 1, O_DEFAULT, 1, 0), (F32, 0, 4, 4844421120, 0, 0, 1)),
    ((49280, 2, 0, O_DEFAULT, 1, 1), (F64, 0, 8, 9739304960, 0, 0, 0)),  # ns > 1 && np > 49152: doubles ...
    ((49280, 2, 0, O_SPLIT, 1, 1), (F64, 0, 8, 9739304960, 0, 0, 0)),    # ... before split is looked at
    ((49280, 2, 0, O_SPLIT, 0, 0), (F64, 0, 8, 9739304960, 0, 0, 0)),
    ((49280, 2, 1, O_DEFAULT, 1, 1), (F32, 0, 4, 4869652480, 0, 0, 0)),  # (f32 comes first)
    ((49280, 1, 0, O_DEFAULT, 1, 1), (MIXED, 1, 6, 7304553472, 0, 1, 1)),  # one right-hand side: no such limit on the storage
    ((49280, 1, 0, O_SPLIT, 1, 1), (SPLIT, 0, 6, 7304478720, 0, 0, 0)),
]


@pytest.mark.parametrize("args,expected", STORAGE_ROWS)
def test_storage_plan(dump, args, expected):
    mode, read32, elt, nbytes, diag_float, want_rowsum, owns_fi = expected
    np_ = args[0]
    assert dump("storage", *args, 36, 32, 8) == dict(mode=mode, read32=read32, fix_bits=36, nib_period=32 * read32, nib_ramp=8 * read32, element_bytes=elt,
                                                     bytes=nbytes, diag_float=diag_float, want_rowsum=want_rowsum, offset_form=int(np_ >= 2048), owns_fi=owns_fi)


def test_storage_plan_carries_the_knobs(dump):
    corrected, uncorrected = (2048, 1, 0, O_DEFAULT, 1, 1), (2048, 1, 0, O_DEFAULT, 1, 0)
    p = dump("storage", *corrected, 32, 16, 0)
    assert (p["fix_bits"], p["read32"], p["nib_period"], p["nib_ramp"]) == (32, 1, 16, 0)
    p = dump("storage", *corrected, 36, 0, 8)                                   # LPVS_NIB_PERIOD=0: no stale nibble product
    assert (p["read32"], p["nib_period"], p["nib_ramp"]) == (1, 0, 8)
    p = dump("storage", *uncorrected, 24, 16, 4)
    assert (p["fix_bits"], p["read32"], p["nib_period"], p["nib_ramp"]) == (24, 0, 0, 0)


def test_a_demoted_plan_is_split_in_the_same_buffer(dump):
    assert dump("demoted", 2048, 1, 0, O_DEFAULT, 1, 1, 36, 32, 8) == dict(mode=SPLIT, read32=1, fix_bits=36, nib_period=0, nib_ramp=8, element_bytes=6,
                                                                            bytes=13369856, diag_float=0, want_rowsum=0, offset_form=1, owns_fi=0)
    assert dump("demoted", 2048, 2, 0, O_DEFAULT, 1, 1, 36, 32, 8)["diag_float"] == 0


@pytest.mark.parametrize("args,repack", [
    ((1, MIXED, 36, 0, MIXED, 36), 0),     # valid, same mode
    ((1, SPLIT, 36, 0, SPLIT, 32), 0),     # (fix bits say nothing about the other storages)
    ((1, SPLIT, 36, 1, MIXED, 36), 0),     # valid, demoted split while mixed is wanted: the second init does not try again
    ((1, SPLIT, 36, 1, MIXED, 32), 0),
    ((1, SPLIT, 36, 0, MIXED, 36), 1),     # a split copy that was asked for by name is not the mixed one
    ((1, SPLIT, 36, 1, F64, 36), 1),       # demoted, another storage wanted
    ((1, MIXED, 36, 0, MIXED, 32), 1),     # valid mixed with other fix bits
    ((1, MIXED, 32, 0, MIXED, 36), 1),
    ((0, MIXED, 36, 0, MIXED, 36), 1),     # not valid
    ((0, SPLIT, 36, 1, MIXED, 36), 1),     # not valid (a new M): the demotion is forgotten
    ((0, NONE, 36, 0, F32, 36), 1),        # the first init
    ((1, MIXED, 36, 0, SPLIT, 36), 1),     # other mode
    ((1, F64, 36, 0, MIXED, 36), 1),
    ((1, F32, 36, 0, F32, 36), 0),
])
def test_must_repack(dump, args, repack):
    assert dump("repack", *args)["repack"] == repack


def test_demote_to_split(dump):
    """2 * fixed < tiles: of 136 tiles 67 fixed-point ones are demoted (134 < 136), 68 are not (136 < 136 is false)."""
    assert dump("demote", 0, 136)["demote"] == 1
    assert dump("demote", 67, 136)["demote"] == 1
    assert dump("demote", 68, 136)["demote"] == 0
    assert dump("demote", 136, 136)["demote"] == 0
    assert dump("demote", 1, 3)["demote"] == 1 and dump("demote", 2, 3)["demote"] == 0         # an odd count: 1.5 is the line


def test_knob_parsers(dump):
    assert dump("knobs") == dict(period=32, ramp=8, fix_bits=36)
    assert dump("knobs", "LPVS_NIB_PERIOD=16", "LPVS_NIB_RAMP=4", "LPVS_FIX_BITS=32") == dict(period=16, ramp=4, fix_bits=32)
    assert dump("knobs", "LPVS_NIB_PERIOD=0", "LPVS_NIB_RAMP=0", "LPVS_FIX_BITS=0") == dict(period=0, ramp=0, fix_bits=36)
    assert dump("knobs", "LPVS_NIB_PERIOD=-3", "LPVS_NIB_RAMP=x", "LPVS_FIX_BITS=x") == dict(period=0, ramp=0, fix_bits=36)
    assert [dump("knobs", f"LPVS_FIX_BITS={b}")["fix_bits"] for b in (19, 20, 36, 37)] == [36, 20, 36, 36]


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
L1, L0, BALL, GROUP = 1, 2, 3, 4                              # LPVS_PROX_*
FACTS = ("np", "n", "ns", "prox", "group_len", "two", "packed", "partials", "offset", "formats", "split", "f32", "fi", "ctl", "scratch", "nrhs", "nbatch")
# a corrected handle of n = 2048 on the mixed storage; cfg2's handle (n = 1024, the full matrix); a pass of 64 windows of np = 512
HANDLE = dict(np=2048, n=2048, ns=1, prox=L1, group_len=0, two=0, packed=1, partials=1, offset=1, formats=1, split=1, f32=0, fi=1, ctl=0, scratch=1, nrhs=1, nbatch=0)
SMALL = dict(np=1024, n=1024, ns=1, prox=L1, group_len=0, two=0, packed=0, partials=1, offset=0, formats=0, split=0, f32=0, fi=0, ctl=1, scratch=1, nrhs=1, nbatch=0)
BATCH = dict(np=512, n=511, ns=64, prox=L1, group_len=0, two=0, packed=1, partials=1, offset=1, formats=1, split=1, f32=0, fi=1, ctl=0, scratch=0, nrhs=1, nbatch=64)


def kind(dump, base, **flip):
    f = dict(base, **flip)
    out = dump("iter", *[f[k] for k in FACTS])
    expect = {ONE_LAUNCH: out["one"], SMALL_ONE_LAUNCH: out["small"], BATCH_ONE_LAUNCH: out["batch"]}
    assert out["kind"] == TWO_LAUNCH or expect[out["kind"]] == 1
    return out["kind"]


HANDLE_ROWS = [
    (dict(), ONE_LAUNCH),
    (dict(two=1), TWO_LAUNCH), (dict(fi=0), TWO_LAUNCH), (dict(ns=2), TWO_LAUNCH), (dict(formats=0), TWO_LAUNCH), (dict(formats=0, split=0, f32=1), ONE_LAUNCH),
    (dict(offset=0), TWO_LAUNCH), (dict(partials=0), TWO_LAUNCH), (dict(packed=0), TWO_LAUNCH),
    (dict(prox=L0), ONE_LAUNCH), (dict(prox=BALL), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=16), ONE_LAUNCH), (dict(prox=GROUP, group_len=128), ONE_LAUNCH),
    (dict(prox=GROUP, group_len=96, n=1920), TWO_LAUNCH),     # 96 divides n = 1920 but not 128: a group would straddle two row blocks
    (dict(prox=GROUP, group_len=256), TWO_LAUNCH), (dict(prox=GROUP, group_len=257, n=2056, np=2176), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=16, n=2040), TWO_LAUNCH),     # n % group_len = 8
    (dict(np=49152, n=49152), ONE_LAUNCH), (dict(np=49280, n=49280), TWO_LAUNCH),
]
SMALL_ROWS = [
    (dict(), SMALL_ONE_LAUNCH),
    (dict(two=1), TWO_LAUNCH), (dict(ctl=0), TWO_LAUNCH), (dict(packed=1), TWO_LAUNCH), (dict(scratch=0), TWO_LAUNCH), (dict(offset=1), TWO_LAUNCH),
    (dict(ns=2), SMALL_ONE_LAUNCH),
    (dict(np=2048, n=2048), SMALL_ONE_LAUNCH), (dict(np=2176, n=2176), TWO_LAUNCH), (dict(np=128, n=100), SMALL_ONE_LAUNCH), (dict(np=64, n=64), TWO_LAUNCH),
    (dict(prox=L0), SMALL_ONE_LAUNCH), (dict(prox=BALL), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=16), SMALL_ONE_LAUNCH),
    (dict(prox=GROUP, group_len=96, n=960), SMALL_ONE_LAUNCH),   # the small kernel's groups need not divide 128
    (dict(prox=GROUP, group_len=256), SMALL_ONE_LAUNCH), (dict(prox=GROUP, group_len=257, n=1028, np=1152), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=0), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=16, n=1000), TWO_LAUNCH),        # n % group_len = 8
]
BATCH_ROWS = [
    (dict(), BATCH_ONE_LAUNCH),
    (dict(two=1), TWO_LAUNCH), (dict(fi=0), TWO_LAUNCH), (dict(nrhs=2), TWO_LAUNCH), (dict(split=0), TWO_LAUNCH), (dict(formats=0), TWO_LAUNCH),
    (dict(offset=0), TWO_LAUNCH), (dict(partials=0), TWO_LAUNCH), (dict(packed=0), TWO_LAUNCH),
    (dict(prox=L0), BATCH_ONE_LAUNCH), (dict(prox=BALL), TWO_LAUNCH),
    (dict(prox=GROUP, group_len=7), TWO_LAUNCH),                 # 511 = 7 * 73, but 7 does not divide 128
    (dict(prox=GROUP, group_len=16, n=512), BATCH_ONE_LAUNCH), (dict(prox=GROUP, group_len=96, n=480), TWO_LAUNCH),
    (dict(np=8192, n=8192), BATCH_ONE_LAUNCH), (dict(np=8320, n=8320), TWO_LAUNCH),
    (dict(np=8192, n=8192, ns=1 << 24, nbatch=1 << 24), TWO_LAUNCH),                # 2^13 * 2^24 * 8 = 2^40 bytes of state: not below 2^40
    (dict(np=8192, n=8192, ns=(1 << 24) - 1, nbatch=(1 << 24) - 1), BATCH_ONE_LAUNCH),
]


@pytest.mark.parametrize("flip,expected", HANDLE_ROWS)
def test_iteration_kind_of_a_handle(dump, flip, expected):
    assert kind(dump, HANDLE, **flip) == expected


@pytest.mark.parametrize("flip,expected", SMALL_ROWS)
def test_iteration_kind_of_a_small_handle(dump, flip, expected):
    assert kind(dump, SMALL, **flip) == expected


@pytest.mark.parametrize("flip,expected", BATCH_ROWS)
def test_iteration_kind_of_a_batch(dump, flip, expected):
    assert kind(dump, BATCH, **flip) == expected


def test_prox_fusable_on_its_own(dump):
    def fusable(**flip):
        f = dict(HANDLE, **flip)
        return dump("iter", *[f[k] for k in FACTS])["fusable"]
    assert [fusable(prox=p) for p in (L1, L0, BALL)] == [1, 1, 0]
    assert [fusable(prox=GROUP, group_len=g) for g in (1, 2, 16, 64, 128)] == [1, 1, 1, 1, 1]
    assert [fusable(prox=GROUP, group_len=g, n=g * 8) for g in (0, 3, 96, 256, 257)] == [0, 0, 0, 0, 0]
    assert fusable(prox=GROUP, group_len=16, n=2040) == 0
    assert fusable(prox=GROUP, group_len=16, two=1, fi=0, packed=0) == 1     # (the prox and the sizes only)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_closure():
    kinds = {k for rows in (HANDLE_ROWS, SMALL_ROWS, BATCH_ROWS) for _, k in rows}
    assert kinds == {TWO_LAUNCH, ONE_LAUNCH, SMALL_ONE_LAUNCH, BATCH_ONE_LAUNCH}
    modes = {expected[0] for _, expected in STORAGE_ROWS}
    assert modes == {NONE, F64, F32, SPLIT, MIXED}
    assert {args[0] for args, _ in STORAGE_ROWS} == {1920, 2048, 49152, 49280} and {args[3] for args, _ in STORAGE_ROWS} == {0, 1, 2, 3, 4}
    for col in (1, 2, 4, 5):                                  # right-hand sides, f32, multi_fixed_ok, corrected: both values occur
        assert len({args[col] for args, _ in STORAGE_ROWS}) == 2
