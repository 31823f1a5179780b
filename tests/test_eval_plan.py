"""What model evaluation (predict / residual / fva) decides on the host before anything is launched (csrc/eval_plan.h):
the admission of a frequency grid to the type-2 non-uniform FFT, its fine grid, the path `auto` takes, the direct path's accumulator
tiling and the slabs of the sums.  The header has no HIP dependency: a tiny host program is built against it as it is and prints what it
decides; CPU only.  Every expected value is a literal worked from the rules.

    1  admission: progressions from 0 and from D, a perturbed grid, residual phases just under and just over kApMaxResidualPhase
    2  fine grids at Nf = 24, 65, 66, 512, 2100 and the refusal at 2101
    3  the path: auto on both sides of its sample threshold, explicit requests
    4  tiling for nb * nc = 1, 6, 8, 64 (and two shapes that need passes / column blocks); slabs"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: eval_plan_dump MODE ARGUMENT ...  ->  one line of key=value pairs; doubles go in and out as hexadecimal floats (%a)
PROGRAM = r"""
#include "eval_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    std::vector<double> d;
    std::vector<long long> v;
    for (int i = 2; i < argc; ++i) { d.push_back(strtod(argv[i], nullptr)); v.push_back(atoll(argv[i])); }
    const auto need = [&](size_t k) { if (v.size() != k) exit(2); };
    if (mode == "admit") {                // xam w ...
        if (d.size() < 2) return 2;
        const EvalGrid g = eval_admit(std::vector<double>(d.begin() + 1, d.end()), d[0]);
        printf("progression=%d ok=%d twin=%d nf=%d emax=%a a=%a D_hi=%a D_lo=%a eps=", (int)g.progression, (int)g.ok, (int)g.twin, g.nf, g.emax, g.a, g.D_hi, g.D_lo);
        for (size_t i = 0; i < g.eps.size(); ++i) printf(i ? ",%a" : "%a", g.eps[i]);
        printf("\n");
    } else if (mode == "grid") {          // Nf: the grid D (0 .. Nf-1), D = 0.25, max|x| = 1
        need(1);
        std::vector<double> w((size_t)v[0]);
        for (size_t f = 0; f < w.size(); ++f) w[f] = 0.25 * (double)f;
        const EvalGrid g = eval_admit(w, 1.0);
        printf("progression=%d ok=%d nf=%d\n", (int)g.progression, (int)g.ok, g.nf);
    } else if (mode == "path") {          // requested grid_ok M
        need(3);
        printf("path=%d threshold=%lld\n", eval_choose_path((int)v[0], v[1] != 0, v[2]), (long long)kEvalNufftMinSamples);
    } else if (mode == "tiling") {        // nb nc
        need(2);
        const EvalTiling t = eval_tiling(v[0], v[1]);
        printf("tj=%d tc=%d jpasses=%d cblocks=%d acc=%d\n", t.tj, t.tc, t.jpasses, t.cblocks, t.acc);
    } else if (mode == "slabs") {         // M
        need(1);
        printf("slabs=%lld block=%d\n", (long long)eval_sum_slabs(v[0]), kEvalBlock);
    } else return 2;
    return 0;
}
"""

DOUBLES = ("emax", "a", "D_hi", "D_lo")


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


def _arg(a):
    return float(a).hex() if isinstance(a, (float, np.floating)) else str(a)


def _parse(out):
    r = {}
    for item in out.split():
        k, v = item.split("=")
        if k in DOUBLES:
            r[k] = float.fromhex(v)
        elif k == "eps":
            r[k] = [float.fromhex(x) for x in v.split(",") if x]
        else:
            r[k] = int(v)
    return r


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(mode, arguments...) -> the dict the program prints."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("eval_plan")
    src, exe = os.path.join(d, "eval_plan_dump.cpp"), os.path.join(d, "eval_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(mode, *args):
        return _parse(subprocess.check_output([exe, mode] + [_arg(a) for a in args], text=True))
    return run


# ---- 1  admission ------------------------------------------------------------------------------------------------------------------------
def test_progression_from_zero_is_admitted_without_a_twin(dump):
    r = dump("admit", 100.0, *[0.5 * f for f in range(8)])           # binary fractions: no rounding anywhere
    assert (r["progression"], r["ok"], r["twin"], r["nf"]) == (1, 1, 0, 256)
    assert (r["a"], r["D_hi"], r["D_lo"], r["emax"]) == (0.0, 0.5, 0.0, 0.0) and r["eps"] == [0.0] * 8


def test_progression_from_its_step_keeps_the_first_frequency_for_the_rotation(dump):
    r = dump("admit", 100.0, *[0.5 * f for f in range(1, 9)])
    assert (r["progression"], r["ok"], r["twin"], r["nf"]) == (1, 1, 0, 256)
    assert (r["a"], r["D_hi"], r["D_lo"]) == (0.5, 0.5, 0.0)


def test_a_step_that_is_no_double_arrives_in_double_double(dump):
    w = [0.1 * f for f in range(1, 4)]                               # 0.1, 0.2, 0.30000000000000004
    r = dump("admit", 1.0, *w)
    D = (np.longdouble(w[2]) - np.longdouble(w[0])) / 2
    assert r["D_hi"] == float(D) and r["D_lo"] == float(D - np.longdouble(float(D))) and r["a"] == 0.1
    assert r["ok"] == 1 and r["nf"] == 256


def test_perturbed_grid_is_refused(dump):
    w = [0.5 * f for f in range(8)]
    w[2] += 1e-3
    r = dump("admit", 100.0, *w)
    assert (r["progression"], r["ok"], r["nf"]) == (0, 0, 0) and r["emax"] == w[2] - 1.0


@pytest.mark.parametrize("xam,admitted", [(107.0, 1), (108.0, 0)])
def test_residual_phase_on_both_sides_of_the_limit(dump, xam, admitted):
    """One residual of 2^-30 (the end points fix a and D, so eps_2 = 2^-30 exactly): emax * xam = 9.965e-8 at 107, 1.0058e-7 at 108,
    against kApMaxResidualPhase = 1e-7.  Admitted grids with a residual run the twin."""
    w = [0.5 * f for f in range(8)]
    w[2] += 2.0 ** -30
    r = dump("admit", xam, *w)
    assert r["emax"] == 2.0 ** -30 and r["eps"] == [0.0, 0.0, 2.0 ** -30, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert (r["progression"], r["ok"], r["twin"]) == (admitted, admitted, admitted) and r["nf"] == 256 * admitted


def test_one_frequency_or_a_zero_step_is_no_progression(dump):
    assert dump("admit", 1.0, 0.7)["progression"] == 0
    assert dump("admit", 1.0, 0.7, 0.7, 0.7)["progression"] == 0
    assert dump("admit", float("inf"), 0.5, 1.0, 1.5)["progression"] == 0      # a sample at infinity


# ---- 2  fine grids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nf,nf", [(24, 256), (65, 256), (66, 512), (512, 2048), (2100, 8192)])
def test_fine_grid_is_the_smallest_power_of_two_above_3_9_modes(dump, Nf, nf):
    assert dump("grid", Nf) == dict(progression=1, ok=1, nf=nf)


def test_a_grid_beyond_8192_points_is_refused(dump):
    assert dump("grid", 2101) == dict(progression=1, ok=0, nf=0)     # 3.9 * 2101 = 8193.9 > 8192


# ---- 3  the path ---------------------------------------------------------------------------------------------------------------------------
def test_auto_takes_the_nufft_from_its_sample_threshold_on(dump):
    assert dump("path", 0, 1, 4095) == dict(path=1, threshold=4096)
    assert dump("path", 0, 1, 4096)["path"] == 2
    assert dump("path", 0, 0, 1 << 20)["path"] == 1                  # a grid that is not admitted: direct at any size


def test_explicit_paths(dump):
    assert dump("path", 1, 1, 1 << 20)["path"] == 1
    assert dump("path", 2, 1, 1)["path"] == 2                        # asked for: no sample threshold
    assert dump("path", 2, 0, 1 << 20)["path"] == -1                 # refused
    assert dump("path", 3, 1, 4096)["path"] == -1 and dump("path", -1, 1, 4096)["path"] == -1


# ---- 4  tiling and slabs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,nc,want", [
    (1, 1, dict(tj=1, tc=1, jpasses=1, cblocks=1, acc=8)),           # nb * nc = 1 (Fourier)
    (6, 1, dict(tj=6, tc=1, jpasses=1, cblocks=1, acc=8)),           # 6 (coulomb, Nv = 3)
    (8, 1, dict(tj=8, tc=1, jpasses=1, cblocks=1, acc=8)),           # 8 (the benchmark's basis)
    (8, 8, dict(tj=8, tc=8, jpasses=1, cblocks=1, acc=64)),          # 64 (a path of 8 penalties): one pass, one sincos per (sample, frequency)
    (16, 3, dict(tj=8, tc=4, jpasses=2, cblocks=1, acc=32)),         # more basis functions: passes
    (6, 20, dict(tj=6, tc=8, jpasses=1, cblocks=3, acc=64)),         # more columns: column blocks
])
def test_accumulator_tiling(dump, nb, nc, want):
    assert dump("tiling", nb, nc) == want


def test_slabs_of_the_sums(dump):
    assert dump("slabs", 1) == dict(slabs=1, block=256)
    assert dump("slabs", 256)["slabs"] == 1 and dump("slabs", 257)["slabs"] == 2 and dump("slabs", 1 << 20)["slabs"] == 4096
