"""The plan of CLEAN (csrc/clean_plan.h): the threads of the loop's workgroup, where the residual lives, the LDS bytes,
and every refusal with its message.  The header has no HIP dependency: a tiny host program is built against it as it is and prints what
it decides; CPU only.  Every expected value is a literal worked from the rules:
  threads   ceil(Nf / 4) rounded up to a multiple of 64, at least 64, at most 1024;
  residual  LDS (1) where 16 Nf <= 128 KiB = 131072, that is Nf <= 8192; global memory (2) beyond, or when forced;
  lds       1024 bytes of arg-max slots, plus 16 Nf where the residual is in LDS.
The same program is also built with -fsanitize=address,undefined and run over the same shapes (a stand-alone program with its own main)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: clean_plan_dump plan ns Nf gain niter tol force   |   clean_plan_dump sizes who ns Nf   |   clean_plan_dump df who df
#        clean_plan_dump sigma df P0 P1 ..   (a real window with |Wn_m|^2 = P_m; as many values as given, padded with the last to an odd count)
PROGRAM = r"""
#include "clean_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 4) return 2;
    if (!strcmp(argv[1], "plan") && argc == 8) {
        const CleanPlan p = clean_plan(atoll(argv[2]), atoll(argv[3]), atof(argv[4]), atoll(argv[5]), atof(argv[6]), atoi(argv[7]) != 0);
        printf("status=%d threads=%d residual=%d lds=%lld workgroups=%lld\nwhy=%s\n", p.status, p.threads, p.residual, (long long)p.lds_bytes,
               (long long)p.workgroups, p.why.c_str());
        return 0;
    }
    int status = kCleanOk;
    std::string why;
    if (!strcmp(argv[1], "sizes") && argc == 5) {
        const bool ok = clean_check_sizes(argv[2], atoll(argv[3]), atoll(argv[4]), &status, &why);
        printf("status=%d ok=%d\nwhy=%s\n", status, ok ? 1 : 0, why.c_str());
        return 0;
    }
    if (!strcmp(argv[1], "df") && argc == 4) {
        const bool ok = clean_check_df(argv[2], atof(argv[3]), &status, &why);
        printf("status=%d ok=%d\nwhy=%s\n", status, ok ? 1 : 0, why.c_str());
        return 0;
    }
    if (!strcmp(argv[1], "sigma")) {
        std::vector<double> Wn;
        for (int i = 3; i < argc; ++i) { Wn.push_back(sqrt(atof(argv[i]))); Wn.push_back(0.0); }
        while ((Wn.size() / 2) % 2 == 0) { Wn.push_back(Wn[Wn.size() - 2]); Wn.push_back(0.0); }
        const long long Nf = ((long long)(Wn.size() / 2) + 1) / 2;
        printf("%.17g\n", clean_sigma(Wn.data(), Nf, atof(argv[2])));
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


def _build(tmp_path_factory, tag, flags):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp(tag)
    src, exe = os.path.join(d, "clean_plan_dump.cpp"), os.path.join(d, "clean_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR] + flags + [src, "-o", exe])   # (host only: no HIP runtime)

    def run(*args):
        out = subprocess.check_output([exe] + [a if isinstance(a, str) else repr(a) for a in args], text=True)
        r = {}
        for line in out.split("\n"):
            if line.startswith("why="):
                r["why"] = line[4:]
            elif "=" in line:
                for item in line.split():
                    k, v = item.split("=")
                    r[k] = int(v)
            elif line:
                r["value"] = float(line)
        return r
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build(tmp_path_factory, "clean_plan", ["-O1"])


OK, ARGUMENT, UNSUPPORTED = 0, 1, 2
LDS, GLOBAL = 1, 2
# Nf -> (threads, residual, LDS bytes)
PLAN_TABLE = [
    (2, (64, LDS, 1024 + 32)),
    (64, (64, LDS, 1024 + 1024)),
    (257, (128, LDS, 1024 + 4112)),             # ceil(257 / 4) = 65 -> 128
    (8192, (1024, LDS, 1024 + 131072)),         # the largest whose residual fits 128 KiB
    (8193, (1024, GLOBAL, 1024)),
    (65536, (1024, GLOBAL, 1024)),
    (1 << 20, (1024, GLOBAL, 1024)),
]
# (ns, Nf, gain, niter, tol) -> (status, message)
REFUSALS = [
    ((1, 1, 0.5, 100, 0.0), (ARGUMENT, "clean: Nf must be at least 2, got 1")),
    ((1, (1 << 20) + 1, 0.5, 100, 0.0), (UNSUPPORTED, "clean: 1048577 frequencies are more than 2^20")),
    ((1, 64, 0.5, -1, 0.0), (ARGUMENT, "clean: niter must not be negative, got -1")),
    ((1, 64, 0.5, (1 << 24) + 1, 0.0), (UNSUPPORTED, "clean: 16777217 iterations are more than 2^24")),
    ((1, 64, 0.0, 100, 0.0), (ARGUMENT, "clean: gain must lie in (0, 2), got 0.000000")),
    ((1, 64, 2.0, 100, 0.0), (ARGUMENT, "clean: gain must lie in (0, 2), got 2.000000")),
    ((1, 64, float("nan"), 100, 0.0), (ARGUMENT, "clean: gain must lie in (0, 2), got nan")),
    ((1, 64, 0.5, 100, -0.25), (ARGUMENT, "clean: tol must lie in [0, 1), got -0.250000")),
    ((1, 64, 0.5, 100, 1.0), (ARGUMENT, "clean: tol must lie in [0, 1), got 1.000000")),
    ((0, 64, 0.5, 100, 0.0), (ARGUMENT, "clean: need 1 <= ns <= 65535 (ns = 0)")),
    ((65536, 64, 0.5, 100, 0.0), (ARGUMENT, "clean: need 1 <= ns <= 65535 (ns = 65536)")),
    ((64, 64, 0.5, 1 << 23, 0.0), (UNSUPPORTED, "clean: 64 signals times 8388608 iterations are more than 2^28 picks")),
]


def _check_all(run):
    for Nf, (threads, residual, lds) in PLAN_TABLE:
        for ns in (1, 3):
            r = run("plan", ns, Nf, 0.5, 100, 0.0, 0)
            assert (r["status"], r["threads"], r["residual"], r["lds"], r["workgroups"]) == (OK, threads, residual, lds, ns), (Nf, r)
        r = run("plan", 1, Nf, 0.5, 100, 0.0, 1)                              # the knob: the residual in global memory, nothing else moves
        assert (r["status"], r["threads"], r["residual"], r["lds"]) == (OK, threads, GLOBAL, 1024), (Nf, r)
    r = run("plan", 1, 64, 1.999, 1 << 24, 0.999, 0)                          # the edges that are admitted
    assert r["status"] == OK
    r = run("plan", 1, 64, 0.5, 0, 0.0, 0)
    assert r["status"] == OK
    for args, (status, why) in REFUSALS:
        r = run("plan", *args, 0)
        assert (r["status"], r["why"]) == (status, why), (args, r)
    # the checks the entries without a loop share
    assert run("sizes", "dirty_spectrum", 1, 1)["why"] == "dirty_spectrum: Nf must be at least 2, got 1"
    assert run("sizes", "clean_restore", 1, (1 << 20) + 1) == {"status": UNSUPPORTED, "ok": 0, "why": "clean_restore: 1048577 frequencies are more than 2^20"}
    assert run("sizes", "dirty_spectrum", 3, 1 << 20)["ok"] == 1
    for bad, text in ((0.0, "0.000000"), (-1.0, "-1.000000"), (float("inf"), "inf"), (float("nan"), "nan")):
        r = run("df", "clean", bad)
        assert (r["status"], r["ok"], r["why"]) == (ARGUMENT, 0, f"clean: df must be positive and finite, got {text}"), (bad, r)
    assert run("df", "clean", 2.0 ** -6)["ok"] == 1
    # sigma: |Wn|^2 = 1, 0.75, 0.25: the half-power point is halfway between m = 1 and m = 2; h = 1.5 df
    s = run("sigma", 0.5, 1.0, 0.75, 0.25)["value"]
    assert abs(s - 1.5 * 0.5 * 0.8493218002880191) <= 1e-15
    # a window that never falls below 1/2: h = (2 Nf - 2) df
    s = run("sigma", 0.5, 1.0, 0.9, 0.8)["value"]
    assert abs(s - 2 * 0.5 * 0.8493218002880191) <= 1e-15


def test_plan_literals_and_refusals(plan):
    _check_all(plan)


def test_the_same_program_under_the_sanitizers(tmp_path_factory):
    """clean_plan.h under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone: the same shapes and refusals, clean exits."""
    run = _build(tmp_path_factory, "clean_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check_all(run)
