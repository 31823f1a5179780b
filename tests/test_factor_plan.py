"""Which schedule and which kernels the factorisation runs at a given size under given knobs (csrc/factor_plan.h).
The header has no HIP dependency: a tiny host program is built against it and prints the plan; CPU only.  Every expected plan below is
written out from the rules of the schedule choice, none is computed by asking the header a second way.

    1  the default table: every np from 128 to 32768, alone, under LPVS_FACTOR_SCHEME=steps, batched, without side streams
    2  every knob alone and the interactions the rules imply, at np in {1024, 1152, 2176, 6272, 8192, 12288}
    3  coverage closure: every plan a default run can take at ANY size is one that tests/test_gpu_factor_exact.py runs bit for bit at
       one of its own sizes -- a moved threshold that leaves a production path untested fails here, without a GPU"""
import os
import shutil
import subprocess

import pytest

import _sweep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: factor_plan_dump NP|FIRST:LAST:STEP NBATCH HAVE_AUX [NAME=VALUE ...]  ->  one line of key=value pairs per np
PROGRAM = r"""
#include "factor_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    long first = 0, last = 0, step = 128;
    if (sscanf(argv[1], "%ld:%ld:%ld", &first, &last, &step) != 3) first = last = atol(argv[1]);
    const int nbatch = atoi(argv[2]), have_aux = atoi(argv[3]);
    const auto get = [&](const char *name) -> const char * {
        const size_t len = strlen(name);
        for (int i = 4; i < argc; ++i)
            if (strncmp(argv[i], name, len) == 0 && argv[i][len] == '=') return argv[i] + len + 1;
        return nullptr;
    };
    const lpvs::FactorKnobs knobs = lpvs::factor_knobs_from(get);
    static const char *const level[] = {"single", "two"}, *const schedule[] = {"groups", "steps_depth2", "steps_depth1", "steps_serial"},
                      *const pivot[] = {"mfma", "regs", "sweep64"};
    for (long np = first; np <= last; np += step) {
        const lpvs::FactorPlan p = lpvs::factor_plan(np, nbatch, have_aux != 0, knobs);
        printf("level=%s schedule=%s kw_outer=%d pivot=%s fused_chain=%d group_max=%d ru_stage=%d band_tile=%d pivot_alone=%d\n", level[(int)p.level],
               schedule[(int)p.schedule], p.kw_outer, pivot[(int)p.pivot], (int)p.fused_chain, p.group_max, p.ru_stage, p.band_tile, (int)p.pivot_alone);
    }
    return 0;
}
"""


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """plans(np or (first, last), knobs, nbatch=1, have_aux=1) -> the plan, or the list of plans of first, first + 128, ..., last."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("factor_plan")
    src, exe = os.path.join(d, "factor_plan_dump.cpp"), os.path.join(d, "factor_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe]   # (host only: the header must not need the HIP runtime)
    subprocess.check_call(cmd)

    def run(np_, knobs=(), nbatch=1, have_aux=1):
        span = f"{np_[0]}:{np_[1]}:128" if isinstance(np_, tuple) else str(np_)
        out = subprocess.check_output([exe, span, str(nbatch), str(have_aux)] + [f"{k}={v}" for k, v in dict(knobs).items()], text=True)
        got = []
        for line in out.splitlines():
            p = dict(kv.split("=") for kv in line.split())
            got.append({k: (v if k in ("level", "schedule", "pivot") else int(v)) for k, v in p.items()})
        return got if isinstance(np_, tuple) else got[0]
    yield run
    shutil.rmtree(d, ignore_errors=True)


# ---- the expected plans, as literals ------------------------------------------------------------------------------------------------
# A field that a schedule does not read has ONE value: the single-level sweep reads none, the steps schedules read kw_outer and pivot.
SINGLE = dict(level="single", schedule="steps_serial", kw_outer=128, pivot="sweep64", fused_chain=0, group_max=1, ru_stage=16, band_tile=128,
              pivot_alone=0)


def steps(schedule, kw=128, pivot="regs"):
    return dict(SINGLE, level="two", schedule=schedule, kw_outer=kw, pivot=pivot)


def groups(group_max, ru_stage, band_tile, pivot_alone, pivot="mfma", fused_chain=1):
    return dict(level="two", schedule="groups", kw_outer=128, pivot=pivot, fused_chain=fused_chain, group_max=group_max, ru_stage=ru_stage,
                band_tile=band_tile, pivot_alone=pivot_alone)


SERIAL, DEPTH1, DEPTH2 = steps("steps_serial"), steps("steps_depth1"), steps("steps_depth2")
SMALL_GROUPS, MID_GROUPS, LARGE_GROUPS = groups(2, 16, 64, 1), groups(2, 16, 128, 1), groups(4, 8, 128, 0)
DEFAULT_TABLE = [(128, 896, SINGLE), (1024, 1920, DEPTH1), (2048, 8064, SMALL_GROUPS), (8192, 12160, MID_GROUPS), (12288, 32768, LARGE_GROUPS)]
STEPS_TABLE = [(128, 896, SINGLE), (1024, 6016, DEPTH1), (6144, 12160, DEPTH2)]                      # from 12288: 256-wide blocks, see the test
NO_AUX_TABLE = [(128, 896, SINGLE), (1024, 32768, SERIAL)]
ALL_NP = (128, 32768)


def _rows(table):
    rows = [(np_, plan) for first, last, plan in table for np_ in range(first, last + 1, 128)]
    assert [np_ for np_, _ in rows] == list(range(128, 32768 + 1, 128))
    return rows


def _assert_table(got, table):
    rows = _rows(table)
    assert len(got) == len(rows)
    for (np_, want), plan in zip(rows, got):
        assert plan == want, (np_, plan, want)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_default_table(plans):
    _assert_table(plans(ALL_NP), DEFAULT_TABLE)


def test_steps_scheme_table(plans):
    """From np = 12288 the steps schedule takes 256-wide pivot blocks, always extracted and swept; a size that is no multiple of 256 ends
    in a ragged 128-wide block, which pivot_inverse_kernel<128> inverts."""
    table = STEPS_TABLE + [(np_, np_, steps("steps_depth2", 256, "sweep64" if np_ % 256 == 0 else "regs")) for np_ in range(12288, 32768 + 1, 128)]
    _assert_table(plans(ALL_NP, {"LPVS_FACTOR_SCHEME": "steps"}), table)


def test_batches_take_the_single_level_sweep_at_every_size(plans):
    for knobs in ({}, {"LPVS_FACTOR_SCHEME": "steps"}, {"LPVS_KW": "256"}):
        _assert_table(plans(ALL_NP, knobs, nbatch=2), [(128, 32768, SINGLE)])


def test_without_side_streams_the_steps_run_serially(plans):
    _assert_table(plans(ALL_NP, have_aux=0), NO_AUX_TABLE)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
NPS = [1024, 1152, 2176, 6272, 8192, 12288]
DEFAULT_AT = {1024: DEPTH1, 1152: DEPTH1, 2176: SMALL_GROUPS, 6272: SMALL_GROUPS, 8192: MID_GROUPS, 12288: LARGE_GROUPS}
STEPS_AT = {1024: DEPTH1, 1152: DEPTH1, 2176: DEPTH1, 6272: DEPTH2, 8192: DEPTH2, 12288: steps("steps_depth2", 256, "sweep64")}
STEPS = {"LPVS_FACTOR_SCHEME": "steps"}


def _kw256(schedule_small, schedule_large, pivot128="regs"):
    """256-wide blocks: 1152, 2176 and 6272 end in a ragged 128-wide block, the other three sizes have none (pivot keeps its fixed value)."""
    return {1024: steps(schedule_small, 256, "sweep64"), 1152: steps(schedule_small, 256, pivot128), 2176: steps(schedule_small, 256, pivot128),
            6272: steps(schedule_large, 256, pivot128), 8192: steps(schedule_large, 256, "sweep64"), 12288: steps(schedule_large, 256, "sweep64")}


def _groups_with(**changed):
    return {np_: (dict(p, **changed) if p["schedule"] == "groups" else p) for np_, p in DEFAULT_AT.items()}


CASES = [
    ({}, DEFAULT_AT),
    (STEPS, STEPS_AT),
    ({"LPVS_FACTOR": "sweep64"}, {np_: SINGLE for np_ in NPS}),
    ({"LPVS_FACTOR": "sweep"}, DEFAULT_AT),                                          # (any other value: nothing)
    # the swept pivot leaves the group schedule for the steps; so do 256-wide blocks
    ({"LPVS_PIVOT": "sweep64"}, {np_: dict(STEPS_AT[np_], kw_outer=128, pivot="sweep64") for np_ in NPS}),
    ({"LPVS_KW": "256"}, _kw256("steps_depth1", "steps_depth2")),
    ({"LPVS_KW": "256", "LPVS_PIVOT": "sweep64"}, _kw256("steps_depth1", "steps_depth2", "sweep64")),
    ({"LPVS_KW": "256", "LPVS_PIVOT": "regs"}, _kw256("steps_depth1", "steps_depth2")),
    ({"LPVS_KW": "256", "LPVS_LOOKAHEAD": "0"}, _kw256("steps_serial", "steps_serial")),
    ({"LPVS_KW": "256", "LPVS_LOOKAHEAD": "1"}, _kw256("steps_depth1", "steps_depth1")),
    ({"LPVS_KW": "128"}, DEFAULT_AT),
    ({"LPVS_KW": "128", **STEPS}, {**STEPS_AT, 12288: DEPTH2}),                         # (128-wide blocks at 12288 too)
    # look-ahead: off = serial steps whatever the scheme; depth one only matters to the steps; anything else is automatic
    ({"LPVS_LOOKAHEAD": "0"}, {np_: SERIAL for np_ in NPS}),
    ({"LPVS_LOOKAHEAD": "0", **STEPS}, {**{np_: SERIAL for np_ in NPS}, 12288: steps("steps_serial", 256, "sweep64")}),
    ({"LPVS_LOOKAHEAD": "1"}, DEFAULT_AT),
    ({"LPVS_LOOKAHEAD": "1", **STEPS}, {1024: DEPTH1, 1152: DEPTH1, 2176: DEPTH1, 6272: DEPTH1, 8192: DEPTH1, 12288: steps("steps_depth1", 256, "sweep64")}),
    ({"LPVS_LOOKAHEAD": "2", **STEPS}, STEPS_AT),
    ({"LPVS_LOOKAHEAD": "", **STEPS}, STEPS_AT),
    ({"LPVS_LOOKAHEAD": "2"}, DEFAULT_AT),
    # the register pivot kernel: instead of the matrix-core one under groups, nothing new under steps
    ({"LPVS_PIVOT": "regs"}, _groups_with(pivot="regs")),
    ({"LPVS_PIVOT": "regs", **STEPS}, STEPS_AT),
    ({"LPVS_PIVOT": "mfma"}, DEFAULT_AT),
    ({"LPVS_CHAIN": "split"}, _groups_with(fused_chain=0)),
    ({"LPVS_CHAIN": "fused"}, DEFAULT_AT),
    # group knobs, in range
    ({"LPVS_FACTOR_GROUP": "1"}, _groups_with(group_max=1)),
    ({"LPVS_FACTOR_GROUP": "2"}, _groups_with(group_max=2)),
    ({"LPVS_FACTOR_GROUP": "3"}, _groups_with(group_max=3)),
    ({"LPVS_FACTOR_GROUP": "4"}, _groups_with(group_max=4)),
    ({"LPVS_RU_STAGE": "8"}, _groups_with(ru_stage=8)),
    ({"LPVS_RU_STAGE": "16"}, _groups_with(ru_stage=16)),
    ({"LPVS_BAND_TILE": "64"}, _groups_with(band_tile=64)),
    ({"LPVS_BAND_TILE": "128"}, _groups_with(band_tile=128)),
    ({"LPVS_PIVOT_ALONE": "0"}, _groups_with(pivot_alone=0)),
    ({"LPVS_PIVOT_ALONE": "1"}, _groups_with(pivot_alone=1)),
    ({"LPVS_PIVOT_ALONE": "7"}, _groups_with(pivot_alone=1)),
    ({"LPVS_PIVOT_ALONE": "-1"}, DEFAULT_AT),
    (R.LARGE_DEFAULTS, _groups_with(group_max=4, ru_stage=8, pivot_alone=0)),
    # ... and out of range: the default
    ({"LPVS_FACTOR_GROUP": "5"}, DEFAULT_AT),
    ({"LPVS_FACTOR_GROUP": "0"}, DEFAULT_AT),
    ({"LPVS_KW": "64"}, DEFAULT_AT),
    ({"LPVS_KW": "64", **STEPS}, STEPS_AT),
    ({"LPVS_RU_STAGE": "4"}, DEFAULT_AT),
    ({"LPVS_BAND_TILE": "32"}, DEFAULT_AT),
    # a knob of the interface, not of the plan
    ({"LPVS_RESERVE_CUS": "0"}, DEFAULT_AT),
]


@pytest.mark.parametrize("knobs,expected", CASES, ids=[R.knob_id(k) for k, _ in CASES])
def test_knobs(plans, knobs, expected):
    assert sorted(expected) == NPS
    for np_ in NPS:
        assert plans(np_, knobs) == expected[np_], (np_, knobs)


GROUP_ONLY = [{"LPVS_CHAIN": "split"}, {"LPVS_FACTOR_GROUP": "3"}, {"LPVS_RU_STAGE": "8"}, {"LPVS_BAND_TILE": "64"}, {"LPVS_BAND_TILE": "128"},
              {"LPVS_PIVOT_ALONE": "0"}, {"LPVS_PIVOT_ALONE": "1"}, R.LARGE_DEFAULTS]


@pytest.mark.parametrize("into_steps", [STEPS, {"LPVS_PIVOT": "sweep64"}, {"LPVS_KW": "256"}, {"LPVS_LOOKAHEAD": "0"}], ids=R.knob_id)
@pytest.mark.parametrize("ignored", GROUP_ONLY, ids=R.knob_id)
def test_group_only_knobs_leave_a_steps_plan_equal(plans, into_steps, ignored):
    for np_ in NPS:
        with_, without = plans(np_, dict(into_steps, **ignored)), plans(np_, into_steps)
        assert without["schedule"] != "groups"
        assert with_ == without, (np_, ignored)
        assert {k: with_[k] for k in ("fused_chain", "group_max", "ru_stage", "band_tile", "pivot_alone")} == \
               {k: SINGLE[k] for k in ("fused_chain", "group_max", "ru_stage", "band_tile", "pivot_alone")}


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
# What tests/test_gpu_factor_exact.py runs: (padded size, knob sets), test by test (all on one matrix: nbatch = 1, with side streams).
_SOME = [{}, {"LPVS_PIVOT": "regs"}, {"LPVS_PIVOT": "sweep64"}, {"LPVS_FACTOR": "sweep64"}]
GPU_EXACT_RUNS = (
    [(np_, R.KNOB_SETS) for np_ in (256, 640, 1024, 1152, 2176, 2304, 2560)] +                                         # item 1
    [(6272, [{}, STEPS, dict(STEPS, LPVS_LOOKAHEAD="1"), {"LPVS_KW": "256"}])] +                                        # item 1, depth two
    [(np_, _SOME + [R.LARGE_DEFAULTS]) for np_ in (1152, 2304)] +                                                       # item 2
    [(2304, [{}, {"LPVS_FACTOR_GROUP": "4", "LPVS_RU_STAGE": "8"}, STEPS, {"LPVS_RESERVE_CUS": "0"}])] +                # item 3
    [(np_, _SOME + [{"LPVS_KW": "256"}]) for np_ in (1152, 2304)] +                                                     # item 4
    [(np_, [{}, {"LPVS_PIVOT": "regs"}, {"LPVS_FACTOR": "sweep64"}, R.LARGE_DEFAULTS]) for np_ in (1152, 2304)])        # item 5


def _key(plan):
    return tuple(sorted(plan.items()))


def test_every_default_plan_is_one_the_exact_gpu_tests_run(plans):
    """The exact tests reach np = 6272 at most; the defaults of larger sizes are reached through knob sets at small ones (_sweep_ref.py:
    LARGE_DEFAULTS, LPVS_BAND_TILE=128).  That those knob sets ARE the large defaults is what this test proves: the plan is the whole
    decision, so equal plans launch the same kinds of kernels in the same order.  Zero default plans may stay uncovered."""
    assert [R.padded_size(n) for n in (200, 640, 1000, 1100, 2100, 2300, 2500, 6200)] == [256, 640, 1024, 1152, 2176, 2304, 2560, 6272]
    covered = {}
    for np_, knob_sets in GPU_EXACT_RUNS:
        for knobs in knob_sets:
            covered.setdefault(_key(plans(np_, knobs)), (np_, knobs))
    default = {}
    for nbatch in (1, 2):
        for np_, plan in zip(range(128, 32768 + 1, 128), plans(ALL_NP, nbatch=nbatch)):
            default.setdefault(_key(plan), (np_, nbatch))
    assert len(default) == 5                                      # (the five rows of DEFAULT_TABLE; a batch adds none)
    uncovered = {first: dict(key) for key, first in default.items() if key not in covered}
    assert not uncovered, f"default plans no exact GPU test runs, with the first (np, nbatch) that takes them: {uncovered}"
    # ... and by name: the two that no test size reaches on its own
    assert plans(12288) == plans(2560, dict(R.LARGE_DEFAULTS, LPVS_BAND_TILE="128")) == LARGE_GROUPS
    assert plans(8192) == plans(2560, {"LPVS_BAND_TILE": "128"}) == MID_GROUPS
    assert plans(2048) == plans(2176) == SMALL_GROUPS
