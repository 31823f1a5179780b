"""The plans of the fold statistics (csrc/fold_plan.h): the frequencies a workgroup folds from one staged block of samples
(F), the signals of a pass (TS), the private copies of the count histogram, the LDS bytes, the passes, the workgroups, and every refusal
with its message.  The header has no HIP dependency: a tiny host program is built against it as it is and prints what it decides; CPU
only.  Every expected value is a literal worked from the rules:
  pdm:  LDS = F nfine ((ts + weighted) 8 + 4) bytes, nfine = nbins covers, at most 63 KiB; ts = 1, 2 or 4 (the smallest that holds ns),
        halved while one frequency does not fit; F = 4, halved while the histograms do not fit or fewer than 256 workgroups would be left;
  cent: LDS = F copies ts cells 4 bytes, cells = nbins mbins; ts and F by the same rules with one copy; copies = 1 (the knob: 1, 2 or 4,
        halved while they do not fit).
The same program is also built with -fsanitize=address,undefined and run over the same shapes (a stand-alone program with its own main)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: fold_plan_dump pdm N ns Nf nbins covers unit f..   |   fold_plan_dump cent N ns Nf nbins mbins knob f..   (f: filled with its first entry up to Nf)
#        fold_plan_dump key v..
PROGRAM = r"""
#include "fold_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "key")) {
        for (int i = 2; i < argc; ++i) {
            const double v = atof(argv[i]);
            printf("%llu %.17g\n", fold_key(v), fold_unkey(fold_key(v)));
        }
        return 0;
    }
    if (!strcmp(argv[1], "vbin")) {                                           // vbin mbins ymin ymax y..
        const int mbins = atoi(argv[2]);
        const double ymin = atof(argv[3]), ymax = atof(argv[4]);
        for (int i = 5; i < argc; ++i) printf("%d\n", cent_value_bin(atof(argv[i]), ymin, ymax - ymin, mbins));
        return 0;
    }
    if (argc < 9) return 2;
    const long long N = atoll(argv[2]), ns = atoll(argv[3]), Nf = atoll(argv[4]), a = atoll(argv[5]), b = atoll(argv[6]), c = atoll(argv[7]);
    std::vector<double> f;
    for (int i = 8; i < argc; ++i) f.push_back(atof(argv[i]));
    if (Nf > (long long)f.size() && Nf <= (1 << 24)) f.resize((size_t)Nf, f[0]);
    if (!strcmp(argv[1], "pdm")) {
        const PdmPlan p = pdm_plan(N, ns, f.data(), Nf, a, b, c != 0);
        printf("status=%d F=%d ts=%d passes=%d unit=%d log2n=%d nfine=%d copies=1 lds=%lld workgroups=%lld\nwhy=%s\n", p.status, p.F, p.ts, p.passes, p.unit,
               p.log2n, p.nfine, (long long)p.lds_bytes, (long long)p.workgroups, p.why.c_str());
    } else {
        const CentPlan p = cent_plan(N, ns, f.data(), Nf, a, b, c);
        printf("status=%d F=%d ts=%d passes=%d cells=%d copies=%d lds=%lld workgroups=%lld\nwhy=%s\n", p.status, p.F, p.ts, p.passes, p.cells, p.copies,
               (long long)p.lds_bytes, (long long)p.workgroups, p.why.c_str());
    }
    return 0;
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
    src, exe = os.path.join(d, "fold_plan_dump.cpp"), os.path.join(d, "fold_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR] + flags + [src, "-o", exe])   # (host only: no HIP runtime)

    def run(which, N, ns, Nf, a, b, c=0, f=(1.0,)):
        args = [which, N, ns, Nf, a, b, int(c)] + [repr(float(x)) for x in np.atleast_1d(f)]
        out = subprocess.check_output([exe] + [str(x) for x in args], text=True)
        r = {}
        for line in out.split("\n"):
            if line.startswith("why="):
                r["why"] = line[4:]
            elif line:
                for item in line.split():
                    k, v = item.split("=")
                    r[k] = int(v)
        return r
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build(tmp_path_factory, "fold_plan", ["-O1"])


OK, ARGUMENT, UNSUPPORTED = 0, 1, 2
# (N, Nf, nbins, covers, ns, unit) -> (F, ts, LDS bytes, passes)
PDM_TABLE = [
    ((1, 1, 2, 1, 1, True), (1, 1, 24, 1)),
    ((255, 70, 5, 2, 3, False), (1, 4, 440, 1)),
    ((1500, 70, 10, 1, 1, True), (1, 1, 120, 1)),
    ((256, 70, 100, 1, 5, False), (1, 4, 4400, 2)),
    ((257, 1030, 8, 4, 2, True), (4, 2, 2560, 1)),
    ((1500, 1030, 512, 4, 1, True), (2, 1, 49152, 1)),       # 4 x 2048 x 12 = 98304 > 64512
    ((1500, 70, 512, 4, 3, False), (1, 2, 57344, 2)),        # four signals: 2048 x 44 = 90112 > 64512; two: 2048 x 28
    ((1500, 1030, 10, 1, 3, False), (4, 4, 1760, 1)),
    ((1500, 1020, 10, 1, 1, True), (2, 1, 240, 1)),          # ceil(1020 / 4) = 255 < 256
    ((1500, 510, 10, 1, 1, True), (1, 1, 120, 1)),           # ceil(510 / 2) = 255 < 256
    ((1 << 18, 65536, 128, 1, 1, False), (4, 1, 10240, 1)),
    ((1 << 18, 65536, 5, 2, 1, False), (4, 1, 800, 1)),
    ((1 << 20, 65536, 1024, 1, 7, False), (1, 4, 45056, 2)), # 2 x 1024 x 44 = 90112 > 64512
]
# (N, Nf, nbins, mbins, ns, knob) -> (F, ts, copies, LDS bytes, passes)
CENT_TABLE = [
    ((1, 1, 2, 2, 1, 0), (1, 1, 1, 16, 1)),
    ((1500, 70, 10, 5, 1, 0), (1, 1, 1, 200, 1)),
    ((1500, 70, 10, 5, 1, 1), (1, 1, 1, 200, 1)),
    ((1500, 70, 10, 5, 1, 2), (1, 1, 2, 400, 1)),
    ((1500, 70, 10, 5, 1, 4), (1, 1, 4, 800, 1)),
    ((1500, 70, 10, 5, 1, 3), (1, 1, 1, 200, 1)),            # a knob that is not 1, 2 or 4 is ignored
    ((255, 1030, 20, 8, 3, 0), (4, 4, 1, 10240, 1)),
    ((255, 1030, 20, 8, 3, 4), (4, 4, 4, 40960, 1)),
    ((256, 1030, 64, 64, 5, 0), (1, 2, 1, 32768, 3)),        # four signals: 4 x 4096 x 4 = 65536 > 64512; F = 2: 65536 again
    ((257, 70, 256, 32, 1, 0), (1, 1, 1, 32768, 1)),
    ((1500, 1030, 64, 64, 1, 0), (2, 1, 1, 32768, 1)),       # F = 4: 65536 > 64512
    ((1500, 1030, 64, 64, 1, 4), (2, 1, 1, 32768, 1)),       # the knob is halved while the copies do not fit: 4 -> 2 (65536) -> 1
    ((1500, 1030, 20, 20, 3, 4), (4, 4, 2, 51200, 1)),       # 400 cells: 4 copies 102400 > 64512, two 51200
    ((1 << 18, 65536, 64, 16, 1, 0), (4, 1, 1, 16384, 1)),
]


def _pdm_expected(N, Nf, nbins, covers, ns, unit):
    nfine = nbins * covers
    lds = lambda F, ts: F * nfine * ((ts + (0 if unit else 1)) * 8 + 4)     # noqa: E731
    ts = 1 if ns <= 1 else 2 if ns == 2 else 4
    while ts > 1 and lds(1, ts) > 63 * 1024:
        ts >>= 1
    F = 4
    while F > 1 and (lds(F, ts) > 63 * 1024 or -(-Nf // F) < 256):
        F >>= 1
    return F, ts, lds(F, ts), -(-ns // ts)


def _cent_expected(N, Nf, nbins, mbins, ns, knob):
    cells = nbins * mbins
    lds = lambda F, copies, ts: F * copies * ts * cells * 4                 # noqa: E731
    ts = 1 if ns <= 1 else 2 if ns == 2 else 4
    while ts > 1 and lds(1, 1, ts) > 63 * 1024:
        ts >>= 1
    F = 4
    while F > 1 and (lds(F, 1, ts) > 63 * 1024 or -(-Nf // F) < 256):
        F >>= 1
    copies = knob if knob in (2, 4) else 1
    while copies > 1 and lds(F, copies, ts) > 63 * 1024:
        copies >>= 1
    return F, ts, copies, lds(F, copies, ts), -(-ns // ts)


@pytest.mark.parametrize("shape,want", PDM_TABLE)
def test_pdm_frequencies_per_workgroup_signals_per_pass_lds_and_passes(plan, shape, want):
    N, Nf, nbins, covers, ns, unit = shape
    assert _pdm_expected(*shape) == want, "the literal does not follow the stated rules"
    r = plan("pdm", N, ns, Nf, nbins, covers, unit)
    assert r["status"] == OK and (r["F"], r["ts"], r["lds"], r["passes"]) == want, r
    assert r["lds"] <= 63 * 1024 and r["workgroups"] == -(-Nf // r["F"]) and r["unit"] == int(unit) and r["nfine"] == nbins * covers
    assert r["log2n"] == (int(np.ceil(np.log2(N))) if N > 1 else 0)


@pytest.mark.parametrize("shape,want", CENT_TABLE)
def test_cent_frequencies_per_workgroup_signals_per_pass_copies_lds_and_passes(plan, shape, want):
    N, Nf, nbins, mbins, ns, knob = shape
    assert _cent_expected(*shape) == want, "the literal does not follow the stated rules"
    r = plan("cent", N, ns, Nf, nbins, mbins, knob)
    assert r["status"] == OK and (r["F"], r["ts"], r["copies"], r["lds"], r["passes"]) == want, r
    assert r["lds"] <= 63 * 1024 and r["workgroups"] == -(-Nf // r["F"]) and r["cells"] == nbins * mbins


def test_the_cases_of_the_gpu_file_have_the_plans_it_asserts(plan):
    from _fold_ref import CENT_CASES, PDM_CASES
    for N, Nf, nbins, covers, ns, weighted, center, want in PDM_CASES.values():
        r = plan("pdm", N, ns, Nf, nbins, covers, not weighted)
        assert (r["F"], r["ts"], r["passes"]) == want
    for N, Nf, nbins, mbins, ns, want in CENT_CASES.values():
        r = plan("cent", N, ns, Nf, nbins, mbins, 0)
        assert (r["F"], r["ts"], r["passes"], r["copies"]) == want
    assert {c[-1][0] for c in PDM_CASES.values()} == {1, 2, 4} == {c[-1][1] for c in PDM_CASES.values()}
    assert {c[-1][0] for c in CENT_CASES.values()} == {1, 2, 4} == {c[-1][1] for c in CENT_CASES.values()} and {c[-1][3] for c in CENT_CASES.values()} == {1}


def test_refusals_and_their_messages(plan):
    for who, which, a, b in (("pdm", "pdm", 10, 1), ("conditional_entropy", "cent", 10, 5)):
        for N, ns, nf in ((0, 1, 2), (10, 0, 2), (10, 65536, 2), (10, 1, 0), (-1, 1, 2)):
            r = plan(which, N, ns, nf, a, b, f=[1.0, 2.0])
            assert r["status"] == ARGUMENT and r["why"] == f"{who}: need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = {N}, Nf = {nf}, ns = {ns})", r
        assert plan(which, 10, 65535, 1, a, b)["status"] == OK
        r = plan(which, (1 << 30) + 1, 1, 1, a, b)
        assert r["status"] == UNSUPPORTED and r["why"] == f"{who}: {(1 << 30) + 1} samples are more than 2^30"
        assert plan(which, 1 << 30, 1, 1, a, b)["status"] == OK
        big = (1 << 24) + 1
        r = plan(which, 10, 1, big, a, b)
        assert r["status"] == UNSUPPORTED and r["why"] == f"{who}: {big} frequencies are more than 2^24"
        for bad in (np.nan, np.inf, -np.inf):
            r = plan(which, 10, 1, 2, a, b, f=[1.0, bad])
            assert r["status"] == ARGUMENT and r["why"] == f"{who}: a frequency is not finite"
        for bad in (0.0, -0.5):
            assert plan(which, 10, 1, 2, a, b, f=[1.0, bad])["why"] == f"{who}: frequency 1 is not positive"
    for nb in (1, 0, -3):
        r = plan("pdm", 10, 1, 1, nb, 1)
        assert r["status"] == ARGUMENT and r["why"] == f"pdm: nbins must be at least 2, got {nb}"
    for nc in (0, -1):
        assert plan("pdm", 10, 1, 1, 10, nc)["why"] == f"pdm: covers must be at least 1, got {nc}"
    for nb, nc in ((2049, 1), (1025, 2), (2, 1025), (100000, 100000)):
        r = plan("pdm", 10, 1, 1, nb, nc)
        assert r["status"] == ARGUMENT and r["why"] == f"pdm: nbins covers must lie in 2 .. 2048, got {nb} x {nc}"
    assert plan("pdm", 10, 1, 1, 2048, 1)["status"] == OK and plan("pdm", 10, 1, 1, 2, 1024)["status"] == OK and plan("pdm", 10, 1, 1, 2, 1)["status"] == OK
    for nb in (1, 257, -2):
        assert plan("cent", 10, 1, 1, nb, 5)["why"] == f"conditional_entropy: nbins must lie in 2 .. 256, got {nb}"
    for mb in (1, 65, 0):
        assert plan("cent", 10, 1, 1, 10, mb)["why"] == f"conditional_entropy: mbins must lie in 2 .. 64, got {mb}"
    r = plan("cent", 10, 1, 1, 256, 33)
    assert r["status"] == ARGUMENT and r["why"] == "conditional_entropy: nbins mbins must be at most 8192, got 256 x 33"
    assert plan("cent", 10, 1, 1, 256, 32)["status"] == OK and plan("cent", 10, 1, 1, 128, 64)["status"] == OK and plan("cent", 10, 1, 1, 2, 2)["status"] == OK


def test_the_key_orders_doubles_as_unsigned_integers_and_comes_back(plan):
    v = [-np.inf, -1e308, -3.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 1e308, np.inf]
    out = subprocess.check_output([plan.exe, "key"] + [repr(float(x)) for x in v], text=True).split("\n")
    keys = [int(line.split()[0]) for line in out if line]
    back = [float(line.split()[1]) for line in out if line]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and all(0 <= k < 2 ** 64 for k in keys)
    assert np.array_equal(np.array(back), np.array(v)) and np.signbit(back[4]) and not np.signbit(back[5])


def test_the_value_bin_at_the_edges(plan):
    def vbin(mbins, ymin, ymax, ys):
        out = subprocess.check_output([plan.exe, "vbin", str(mbins), repr(float(ymin)), repr(float(ymax))] + [repr(float(x)) for x in ys], text=True)
        return [int(x) for x in out.split()]
    assert vbin(5, 0, 4, [0, 1, 2, 3, 4]) == [0, 1, 2, 3, 4]                   # u 5 = 0, 1.25, 2.5, 3.75, 5 -> the last bin
    assert vbin(4, 0, 4, [0, 1, 2, 3, 4]) == [0, 1, 2, 3, 3]                   # u 4 = y exactly: a tie at an edge goes up, ymax into the last bin
    assert vbin(5, 3.7, 3.7, [3.7]) == [0]                                     # a constant signal
    assert vbin(64, -1e308, 1e308, [-1e308, 0.0, 1e308]) == [0, 0, 0]          # ymax - ymin overflows: every sample in bin 0


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """A stand-alone host program with its own main, built with -fsanitize=address,undefined and run over the tables' shapes and every
    kind of refusal: any report makes the program exit non-zero (-fno-sanitize-recover)."""
    run = _build(tmp_path_factory, "fold_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for shape, want in PDM_TABLE:
        N, Nf, nbins, covers, ns, unit = shape
        r = run("pdm", N, ns, Nf, nbins, covers, unit)
        assert (r["F"], r["ts"], r["lds"], r["passes"]) == want
    for shape, want in CENT_TABLE:
        N, Nf, nbins, mbins, ns, knob = shape
        r = run("cent", N, ns, Nf, nbins, mbins, knob)
        assert (r["F"], r["ts"], r["copies"], r["lds"], r["passes"]) == want
    assert run("pdm", 0, 1, 1, 10, 1)["status"] == ARGUMENT and run("pdm", 10, 1, 2, 10, 1, f=[1.0, np.nan])["status"] == ARGUMENT
    assert run("pdm", 10, 1, 1, 100000, 100000)["status"] == ARGUMENT and run("cent", 10, 1, 1, 256, 33)["status"] == ARGUMENT
    assert run("cent", 10, 1, (1 << 24) + 1, 10, 5)["status"] == UNSUPPORTED and run("pdm", (1 << 30) + 1, 1, 1, 10, 1)["status"] == UNSUPPORTED
    subprocess.check_call([run.exe, "key", "-inf", "-0.0", "0.0", "inf", "1e308"])
    subprocess.check_call([run.exe, "vbin", "64", "-1e308", "1e308", "0.0", "1e308"])
