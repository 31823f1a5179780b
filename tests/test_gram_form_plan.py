"""What the problem constructors and the window engine decide on the host before any Gram is built (csrc/gram_form_plan.h; DESIGN.md
4.2, 4.6): the slot tables and the admission of a frequency grid, the basis centres, the limits of the non-uniform FFT, the form
decision, the dense plan and the flop counts.  The header has no HIP dependency: a tiny host program is built against it and prints
what it decides; CPU only.  Every expected value below is a literal worked from the rules, none is computed by asking the header a
second way (the grids whose step is not a binary fraction are checked against rational arithmetic instead).

    1  slot tables: layout and admission, case by case; the table entries; the right-hand-side helpers
    2  basis centres, the zero-frequency rule
    3  limits of the non-uniform FFT
    4  the form decision: one row per clause, and every form occurs
    5  dense plan: tiles, split, LDS images and stage depths, the pair form's limit, flop counts
    6  the same program under AddressSanitizer and UBSan, once over all cases"""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: gram_form_plan_dump MODE ARGUMENT ...  ->  one line of key=value pairs; doubles go in and out as hexadecimal floats (%a), lists
# are comma-separated
PROGRAM = r"""
#include "gram_form_plan.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace lpvs;
static void dlist(const char *key, const double *p, size_t n) {
    printf("%s=", key);
    for (size_t i = 0; i < n; ++i) printf(i ? ",%a" : "%a", p[i]);
    printf(" ");
}
static void dlist(const char *key, const std::vector<double> &v) { dlist(key, v.data(), v.size()); }
static void tlist(const std::vector<GramTile> &t) {
    printf("tile_list=");
    for (size_t i = 0; i < t.size(); ++i) printf(i ? ",%d:%d" : "%d:%d", t[i].i, t[i].j);
    printf("\n");
}
static void plan(const GramPlan &p) {
    printf("n=%lld N=%lld tiles=%lld ksplit=%lld rows_per_chunk=%lld slab_bytes=%zu pairs=%lld np2=%lld issued=%a\n", (long long)p.n, (long long)p.N,
           (long long)p.tiles, (long long)p.ksplit, (long long)p.rows_per_chunk, p.slab_bytes, (long long)p.pairs, (long long)p.np2, dense_issued_flops(p));
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    std::vector<double> d;
    std::vector<long long> v;
    for (int i = 2; i < argc; ++i) { d.push_back(strtod(argv[i], nullptr)); v.push_back(atoll(argv[i])); }
    const auto need = [&](size_t k) { if (v.size() != k) exit(2); };
    if (mode == "slots") {                // f32_grid xam w ...
        if (d.size() < 3) return 2;
        const ApSlots sl = make_ap_slots(std::vector<double>(d.begin() + 2, d.end()), d[1], v[0] != 0);
        printf("ok=%d merged=%d s0=%lld nf8=%lld s8=%lld nsl=%lld emax=%a delta=%a ", (int)sl.ok, (int)sl.merged, (long long)sl.s0, (long long)sl.nf8,
               (long long)sl.s8, (long long)sl.nsl, sl.emax, sl.delta);
        dlist("eps", sl.eps);
        if (sl.ok) {
            dlist("om_hi", sl.om_hi); dlist("om_lo", sl.om_lo); dlist("omr_hi", sl.omr_hi); dlist("omr_lo", sl.omr_lo);
            dlist("step_hi", sl.step.hi, 8); dlist("step_lo", sl.step.lo, 8); dlist("rhs_residuals", rhs_residuals(sl));
            printf("rhs_on_grid=%d", (int)rhs_on_grid(sl));
        }
        printf("\n");
    } else if (mode == "centers") {       // lo hi amax Nv coulomb
        need(5);
        std::vector<double> vc; double gamma = 0;
        basis_centers(d[0], d[1], d[2], v[3], (int)v[4], vc, &gamma);
        dlist("vc", vc); printf("gamma=%a\n", gamma);
    } else if (mode == "freq") {          // f ...
        printf("zerofreq=%lld\n", (long long)check_freq_host(d.data(), (int64_t)d.size()));
    } else if (mode == "nufft") {         // N nslots nq
        need(3);
        printf("grid=%d applicable=%d\n", nufft_grid_size(v[1]), (int)nufft_applicable(v[0], v[1], v[2]));
    } else if (mode == "nufft_windows") { // n nslots
        need(2);
        printf("applicable=%d\n", (int)nufft_windows_applicable(v[0], v[1]));
    } else if (mode == "form") {          // family option slots_ok merged slots_direct N nsl nq nb
        need(9);
        GramFormFacts f;
        f.family = (GramFamily)v[0]; f.option = (int)v[1]; f.slots_ok = v[2] != 0; f.merged = v[3] != 0; f.slots_direct = v[4] != 0;
        f.N = v[5]; f.nsl = v[6]; f.nq = v[7]; f.nb = v[8];
        const GramForm g = choose_gram_form(f);
        printf("form=%d structured=%d wants_slots=%d\n", (int)g, (int)is_structured(g), (int)gram_option_wants_slots(f.option));
    } else if (mode == "plan") {          // n N nbatch
        need(3);
        plan(make_gram_plan(v[0], v[1], v[2]));
    } else if (mode == "plan_pairs") {    // Nf nb N
        need(3);
        plan(make_gram_plan_pairs(v[0], v[1], v[2]));
    } else if (mode == "tiles") {         // n
        need(1);
        tlist(make_tiles(v[0]));
    } else if (mode == "tiles_pairs") {   // np2 P
        need(2);
        tlist(make_tiles_pairs(v[0], v[1]));
    } else if (mode == "stage") {         // mode nb ldk
        need(3);
        printf("stage=%d lds32=%zu lds16=%zu lds8=%zu\n", gram_stage_for((int)v[0], v[1], v[2]), gram_lds_bytes((int)v[0], 32, v[1], v[2]),
               gram_lds_bytes((int)v[0], 16, v[1], v[2]), gram_lds_bytes((int)v[0], 8, v[1], v[2]));
    } else if (mode == "krs_fits") {      // nb
        need(1);
        printf("fits=%d\n", (int)gram_krs_fits(v[0]));
    } else if (mode == "flops") {         // N n nsl nq
        need(4);
        printf("gram=%a structured=%a\n", gram_flops(v[0], v[1]), structured_issued_flops(v[0], v[2], v[3]));
    } else return 2;
    return 0;
}
"""

DOUBLES = ("emax", "delta", "gamma", "issued", "gram", "structured")
DOUBLE_LISTS = ("eps", "om_hi", "om_lo", "omr_hi", "omr_lo", "step_hi", "step_lo", "rhs_residuals", "vc")


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


def _arg(a):
    return float(a).hex() if isinstance(a, (float, np.floating)) else str(a)


def _parse(out):
    kv = dict(item.split("=") for item in out.split())
    r = {}
    for k, v in kv.items():
        if k in DOUBLES:
            r[k] = float.fromhex(v)
        elif k in DOUBLE_LISTS:
            r[k] = [float.fromhex(x) for x in v.split(",") if x]
        elif k == "tile_list":
            r[k] = [tuple(int(q) for q in x.split(":")) for x in v.split(",") if x]
        else:
            r[k] = int(v)
    return r


def _build(tmp_path_factory, name, flags):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp(name)
    src, exe = os.path.join(d, "gram_form_plan_dump.cpp"), os.path.join(d, "gram_form_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe] + flags)   # (host only: no HIP runtime)
    return d, exe


CALLS = []   # every call the tests made: section 6 replays them under the sanitizers


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(mode, arguments...) -> the dict the program prints."""
    d, exe = _build(tmp_path_factory, "gram_form_plan", ["-O1"])

    def run(mode, *args):
        argv = [mode] + [_arg(a) for a in args]
        if argv not in CALLS:
            CALLS.append(argv)
        return _parse(subprocess.check_output([exe] + argv, text=True))
    yield run
    shutil.rmtree(d, ignore_errors=True)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
D = 0.25
NAN, INF = float("nan"), float("inf")


def grid(a, nf=8, step=D):
    return [a + step * f for f in range(nf)]     # (exact: binary fractions)


def bump(w, i, by):
    w = list(w); w[i] += by
    return w


def put(w, i, value):
    w = list(w); w[i] = value
    return w


def slots(dump, w, xam=100.0, f32=0):
    return dump("slots", f32, float(xam), *[float(x) for x in w])


def layout(s):
    return (s["ok"], s["merged"], s["s0"], s["nf8"], s["s8"], s["nsl"])


README_GRID = grid(D)                            # w = D * (1 .. 8)
BUMPED = bump(README_GRID, 3, 2.0 ** -30)        # w[3] = 1 + 2^-30: the end points, and so D, stay


@pytest.mark.parametrize("w,expected,on_grid", [
    (README_GRID, (1, 1, 2, 8, 24, 24), 1),              # 2a = 2 D: j0 = 2, 2 + 15 slots -> 24; the rhs rides the grid at mode 1
    (grid(0.0), (1, 1, 0, 8, 16, 16), 1),                # default_freqs: j0 = 0, 15 slots -> 16
    (grid(D / 2), (1, 1, 1, 8, 16, 16), 0),              # j0 = 1 is odd: a + f D is no multiple of D
    (grid(3.5 * D), (1, 1, 7, 8, 24, 24), 0),            # j0 = 7 = Nf - 1: still merged, 7 + 15 = 22 -> 24
    (grid(4 * D), (1, 0, 8, 8, 16, 24), 1),              # j0 = Nf: split, s0 = nf8, 8 + 16 slots
    (grid(D / 4), (1, 0, 8, 8, 16, 24), 1),              # j0r = 0.5 rounds to 1, delta = -D/2: far beyond the bound
    ([2.0 - D * f for f in range(8)], (1, 0, 8, 8, 16, 24), 1),   # negative step: j0 = -16
    ([D], (1, 0, 8, 8, 8, 16), 1),                       # Nf = 1: D = 0, no merged layout; one sum slot -> 8
    (grid(D, nf=5), (1, 1, 2, 8, 16, 16), 1),            # Nf = 5: nf8 = 8, 2 + 9 = 11 slots -> 16
])
def test_slot_layouts(dump, w, expected, on_grid):
    s = slots(dump, w)
    assert layout(s) == expected and s["delta"] == 0.0 and s["emax"] == 0.0
    assert s["rhs_on_grid"] == on_grid
    assert s["eps"] == [0.0] * len(w) and len(s["om_hi"]) == len(s["om_lo"]) == expected[5] and len(s["omr_hi"]) == 8


def test_admission_bounds(dump):
    eps = [0.0, 0.0, 0.0, 2.0 ** -30, 0.0, 0.0, 0.0, 0.0]
    s = slots(dump, BUMPED, xam=64)                      # 2^-30 * 64 = 5.96e-8 <= 1e-7
    assert layout(s) == (1, 1, 2, 8, 24, 24) and s["emax"] == 2.0 ** -30 and s["eps"] == eps
    s = slots(dump, BUMPED, xam=128)                     # 1.19e-7 > 1e-7
    assert s["ok"] == 0 and s["emax"] == 2.0 ** -30 and s["eps"] == eps and "om_hi" not in s
    # the float-grid admission: residuals up to 2^-23 max|w| = 2^-22; they are kept while their phases are <= 3e-3
    s = slots(dump, BUMPED, xam=128, f32=1)
    assert layout(s) == (1, 1, 2, 8, 24, 24) and s["eps"] == eps
    assert slots(dump, BUMPED, xam=2.0 ** 21, f32=1)["eps"] == eps           # 2^-9 = 1.95e-3
    s = slots(dump, BUMPED, xam=2.0 ** 22, f32=1)                            # 2^-8 = 3.9e-3: snapped grid
    assert layout(s) == (1, 1, 2, 8, 24, 24) and s["eps"] == [0.0] * 8 and s["emax"] == 2.0 ** -30
    assert slots(dump, bump(README_GRID, 3, 2.0 ** -21), xam=128, f32=1)["ok"] == 0   # 2^-21 > 2^-22
    assert slots(dump, BUMPED, xam=2.0 ** 22)["ok"] == 0                     # (and never without the float-grid admission)


def test_admission_of_non_finite_input(dump):
    assert slots(dump, README_GRID, xam=INF)["ok"] == 0
    assert slots(dump, put(README_GRID, 7, INF))["ok"] == 0                  # D = inf: the residuals are inf or NaN, emax = inf
    # A NaN in w is ADMITTED: fmax drops it, emax stays 0.  Known behaviour, pinned as it is.
    s = slots(dump, put(README_GRID, 3, NAN))
    assert layout(s) == (1, 1, 2, 8, 24, 24) and s["emax"] == 0.0
    assert math.isnan(s["eps"][3]) and [e for i, e in enumerate(s["eps"]) if i != 3] == [0.0] * 7
    s = slots(dump, put(README_GRID, 7, NAN))                                # D = NaN: every residual NaN, no merged layout
    assert layout(s) == (1, 0, 8, 8, 16, 24) and s["emax"] == 0.0 and all(math.isnan(e) for e in s["eps"])


def test_slot_table_entries(dump):
    s = slots(dump, README_GRID)                                             # merged: one progression j D
    assert s["om_hi"] == [D * j for j in range(24)] and s["om_lo"] == [0.0] * 24
    assert s["omr_hi"] == [D + D * f for f in range(8)] and s["omr_lo"] == [0.0] * 8
    assert s["step_hi"] == [D * b for b in range(8)] and s["step_lo"] == [0.0] * 8
    s = slots(dump, grid(4 * D))                                             # split: differences m D, then sums 2 a + q D with a = 1
    assert s["om_hi"] == [D * m for m in range(8)] + [2.0 + D * q for q in range(16)] and s["om_lo"] == [0.0] * 24
    assert s["omr_hi"] == [1.0 + D * f for f in range(8)]


def _exact_tables(w):
    """a, step and the residuals of the end-point progression in rational arithmetic."""
    wq = [Fraction(x) for x in w]
    a0, step = wq[0], (wq[-1] - wq[0]) / (len(wq) - 1)
    return wq, a0, step, [wq[f] - (a0 + f * step) for f in range(len(wq))]


def test_double_double_entries_of_an_inexact_step(dump):
    """D = 2 pi 25 / 512 is no binary fraction: the tables carry non-zero low parts, and hi + lo is the RATIONAL value to 2^-100 of it
    (double-double arithmetic; an 80-bit long double would stop at 2^-64)."""
    d0 = 2 * math.pi * 25 / 512
    w = [d0 * k for k in range(1, 9)]
    s = slots(dump, w)
    wq, a0, step, eps = _exact_tables(w)
    tiny = Fraction(1, 2 ** 100)
    assert layout(s) == (1, 1, 2, 8, 24, 24)
    assert all(abs(Fraction(g) - e) <= tiny * wq[-1] for g, e in zip(s["eps"], eps)) and s["emax"] == max(abs(e) for e in s["eps"])
    assert abs(Fraction(s["delta"]) - (2 * a0 - 2 * step)) <= tiny * wq[-1]
    dd = lambda hi, lo: [Fraction(h) + Fraction(l) for h, l in zip(s[hi], s[lo])]       # noqa: E731
    for got, want in ((dd("om_hi", "om_lo"), [j * step for j in range(24)]), (dd("omr_hi", "omr_lo"), [a0 + f * step for f in range(8)]),
                      (dd("step_hi", "step_lo"), [b * step for b in range(8)])):
        assert len(got) == len(want) and all(abs(g - v) <= tiny * abs(v) for g, v in zip(got, want))
    assert s["om_hi"] == [float(j * step) for j in range(24)]
    assert sum(1 for l in s["om_lo"] if l != 0.0) >= 12 and all(abs(l) <= abs(h) * 2.0 ** -53 for h, l in zip(s["om_hi"], s["om_lo"]))


@pytest.mark.parametrize("name,w,xam", [
    ("the benchmark's grid at |w x| = 3e6", [2 * math.pi * k * 25 / 24 for k in range(1, 25)], 2.0e4),
    ("the same from a = 1.37 D: two slot families", [2 * math.pi * (1.37 + k) * 25 / 24 for k in range(24)], 2.0e4),
    ("a Fourier grid k / 97 late in a record, |w x| = 4e7", [6.283185307179586 * (k / 97.0) for k in range(1, 41)], 2.0 ** 24 + 300.0)])
def test_tables_hold_the_real_frequencies_at_large_abscissae(dump, name, w, xam):
    """What the tables put between a kernel and the phase of the real product, in rational arithmetic: slot frequency + first-order
    residuals against w_f - w_f', w_f + w_f' and w_f, times max|x|.  Worked in long double the tables were off by 4.2e-13 rad on the first
    grid and 6.4e-12 rad on the last (2^-64 |w x| per operation), against the 1e-12 the structured forms are held to; in double-double
    what is left is the rounding of the residuals to doubles, 2^-53 max|eps| max|x| < 1e-24."""
    s = slots(dump, w, xam=xam)
    wq = [Fraction(x) for x in w]
    Nf = len(w)
    assert s["ok"] == 1 and s["merged"] == (0 if "1.37" in name else 1)
    eps, delta = [Fraction(e) for e in s["eps"]], Fraction(s["delta"])
    om = [Fraction(h) + Fraction(l) for h, l in zip(s["om_hi"], s["om_lo"])]
    omr = [Fraction(h) + Fraction(l) for h, l in zip(s["omr_hi"], s["omr_lo"])]
    worst = Fraction(0)
    for f in range(Nf):
        worst = max(worst, abs(omr[f] + eps[f] - wq[f]))
        for g in range(Nf):
            if f >= g:
                worst = max(worst, abs(om[f - g] + (eps[f] - eps[g]) - (wq[f] - wq[g])))
            ssum = om[s["s0"] + f + g] + (delta if s["merged"] else 0)
            worst = max(worst, abs(ssum + eps[f] + eps[g] - (wq[f] + wq[g])))
    print(f"{name}: the tables' own phase error {float(worst * Fraction(xam)):.3e} rad")
    assert worst * Fraction(xam) <= Fraction(1, 10 ** 20)


def test_rhs_residuals(dump):
    # a = D + 2^-31: 2a = 2 D + 2^-30, j0 = 2, delta = 2^-30 (phase 5.96e-8 at max|x| = 64); w[3] carries 2^-32 more
    w = bump(grid(D + 2.0 ** -31), 3, 2.0 ** -32)
    s = slots(dump, w, xam=64)
    assert layout(s) == (1, 1, 2, 8, 24, 24) and s["delta"] == 2.0 ** -30 and s["rhs_on_grid"] == 1
    assert s["eps"] == [0.0, 0.0, 0.0, 2.0 ** -32, 0.0, 0.0, 0.0, 0.0]
    assert s["rhs_residuals"] == [2.0 ** -31] * 3 + [2.0 ** -31 + 2.0 ** -32] + [2.0 ** -31] * 4
    assert slots(dump, w, xam=128)["merged"] == 0                            # delta is held to the same bound as the residuals


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_basis_centers(dump):
    assert dump("centers", 0.0, 1.0, 1.0, 5, 0) == dict(vc=[0.0, 0.25, 0.5, 0.75, 1.0], gamma=5.0)
    assert dump("centers", 0.5, 2.0, 2.0, 1, 0) == dict(vc=[0.5], gamma=INF)
    assert dump("centers", -6.0, 3.0, 6.0, 2, 1) == dict(vc=[-4.0, -2.0, 2.0, 4.0], gamma=0.5)


def test_check_freq_host(dump):
    assert dump("freq", 0.0, 1.0, 2.0)["zerofreq"] == 1
    assert dump("freq", 1.0, 0.0, 2.0)["zerofreq"] == -1
    assert dump("freq", 1.0, 2.0, 3.0)["zerofreq"] == 0


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_nufft_limits(dump):
    assert dump("nufft", 4096, 1, 1) == dict(grid=256, applicable=1)
    assert dump("nufft", 4096, 65, 1) == dict(grid=256, applicable=1)        # 3.9 * 65 = 253.5
    assert dump("nufft", 4096, 66, 1) == dict(grid=512, applicable=1)        # 3.9 * 66 = 257.4
    assert dump("nufft", 4096, 2096, 256) == dict(grid=8192, applicable=1)   # 3.9 * 2096 = 8174.4
    assert dump("nufft", 4096, 2104, 256) == dict(grid=16384, applicable=0)  # 3.9 * 2104 = 8205.6
    assert dump("nufft", 4095, 24, 3)["applicable"] == 0
    assert dump("nufft", 4096, 24, 0)["applicable"] == 0
    assert dump("nufft", 4096, 24, 257)["applicable"] == 0
    assert dump("nufft_windows", 2048, 1048)["applicable"] == 1              # 3.9 * 1048 = 4087.2
    assert dump("nufft_windows", 2048, 1056)["applicable"] == 0              # 3.9 * 1056 = 4118.4
    assert dump("nufft_windows", 2047, 72)["applicable"] == 0
    assert dump("nufft_windows", 2048, 56)["applicable"] == 0
    assert dump("nufft_windows", 2048, 64)["applicable"] == 1


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
LPV, FOURIER, WINDOWS = 0, 1, 2
AUTO, AP, KRS, KR = 0, 1, 2, 3
REFUSED, FORM_KR, FORM_KRS, FORM_PANEL, FORM_AP, FORM_AP_NUFFT = 0, 1, 2, 3, 4, 5
#   family   option ok merged direct N     nsl   nq   nb   form
FORM_TABLE = [
    (LPV,     AUTO,  1, 1,     0,     4096, 24,   3,   2,   FORM_AP_NUFFT),
    (LPV,     AUTO,  1, 0,     0,     4096, 24,   3,   2,   FORM_AP),          # split layout
    (LPV,     AUTO,  1, 1,     0,     4095, 24,   3,   2,   FORM_AP),          # the NUFFT limits: samples,
    (LPV,     AUTO,  1, 1,     0,     4096, 2104, 3,   2,   FORM_AP),          # ... grid size,
    (LPV,     AUTO,  1, 1,     0,     4096, 24,   276, 23,  FORM_AP),          # ... weight vectors
    (LPV,     AUTO,  1, 1,     1,     4096, 24,   3,   2,   FORM_AP),          # slot sums: direct
    (LPV,     AP,    1, 1,     0,     4096, 24,   3,   2,   FORM_AP_NUFFT),
    (LPV,     AP,    0, 0,     0,     4096, 0,    3,   2,   REFUSED),
    (LPV,     AUTO,  0, 0,     0,     4096, 0,    3,   2,   FORM_KRS),
    (LPV,     AUTO,  0, 0,     0,     4096, 0,    1,   1,   FORM_KR),          # one basis function has no pairs
    (LPV,     AUTO,  0, 0,     0,     4096, 0,    528, 32,  FORM_KR),          # the pair table does not fit LDS
    (LPV,     KR,    0, 0,     0,     4096, 0,    3,   2,   FORM_KR),
    (LPV,     KR,    1, 1,     0,     4096, 24,   3,   2,   FORM_KR),          # (the grid is not looked at)
    (LPV,     KRS,   0, 0,     0,     4096, 0,    3,   2,   FORM_KRS),
    (LPV,     KRS,   0, 0,     0,     4096, 0,    1,   1,   FORM_KR),
    (FOURIER, AUTO,  1, 1,     0,     4096, 24,   0,   0,   FORM_AP),          # (no NUFFT path)
    (FOURIER, AUTO,  0, 0,     0,     4096, 0,    0,   0,   FORM_PANEL),
    (FOURIER, KRS,   1, 1,     0,     4096, 24,   0,   0,   FORM_PANEL),
    (FOURIER, AP,    0, 0,     0,     4096, 0,    0,   0,   REFUSED),
    (WINDOWS, AUTO,  1, 1,     0,     2048, 72,   0,   0,   FORM_AP_NUFFT),
    (WINDOWS, AUTO,  1, 1,     0,     2047, 72,   0,   0,   FORM_AP),
    (WINDOWS, AUTO,  1, 1,     0,     2048, 56,   0,   0,   FORM_AP),
    (WINDOWS, AUTO,  1, 1,     0,     2048, 1056, 0,   0,   FORM_AP),
    (WINDOWS, AUTO,  1, 0,     0,     2048, 72,   0,   0,   FORM_AP),
    (WINDOWS, AUTO,  1, 1,     1,     2048, 72,   0,   0,   FORM_AP),
    (WINDOWS, AUTO,  0, 0,     0,     2048, 0,    0,   0,   FORM_PANEL),
    (WINDOWS, AP,    0, 0,     0,     2048, 0,    0,   0,   REFUSED),
]


@pytest.mark.parametrize("row", FORM_TABLE)
def test_form_decision(dump, row):
    r = dump("form", *row[:-1])
    assert r["form"] == row[-1] and r["structured"] == int(row[-1] in (FORM_AP, FORM_AP_NUFFT)) and r["wants_slots"] == int(row[1] in (AUTO, AP))


def test_form_table_is_closed():
    assert {row[-1] for row in FORM_TABLE} == {REFUSED, FORM_KR, FORM_KRS, FORM_PANEL, FORM_AP, FORM_AP_NUFFT}
    assert {row[-1] for row in FORM_TABLE if row[0] == LPV} == {REFUSED, FORM_KR, FORM_KRS, FORM_AP, FORM_AP_NUFFT}


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_tiles(dump):
    assert dump("tiles", 300)["tile_list"] == [(0, 0), (1, 0), (2, 0), (2, 1)]   # tile row ti holds the columns tj <= ti / 2
    assert dump("tiles_pairs", 16, 3)["tile_list"] == [(0, 0)]
    # rows p < 200, columns p' * 36 + pair: tile row 0 (p <= 127) needs the tiles whose first column has p' <= 127: tj * 256 / 36 <= 127
    t = dump("tiles_pairs", 200, 36)["tile_list"]
    assert t == [(0, j) for j in range(18)] + [(1, j) for j in range(29)]


def test_dense_plans(dump):
    # one tile; 10 stages of 64 samples allow no split (8 stages per chunk at least)
    assert dump("plan", 12, 600, 1) == dict(n=12, N=600, tiles=1, ksplit=1, rows_per_chunk=640, slab_bytes=262144, pairs=0, np2=0,
                                            issued=2.0 * 128 * 256 * 640)
    # 8 tile rows: 1 + 1 + 2 + 2 + 3 + 3 + 4 + 4 = 20 tiles; 1563 stages allow 195 chunks, 4096 / 20 asks for 205 -> 195; 20 ks fills
    # whole rounds of 256 when 64 | ks: the first in [97, 195] is 128; ceil(100000 / 128) = 782 -> 832
    assert dump("plan", 1000, 100000, 1) == dict(n=1000, N=100000, tiles=20, ksplit=128, rows_per_chunk=832, slab_bytes=8 * 20 * 128 * 128 * 256,
                                                 pairs=0, np2=0, issued=20 * 2.0 * 128 * 256 * 128 * 832)
    # a batch of 64 windows: 32 stages allow 4 chunks; 64 * 4 = 256 items are one whole round
    assert dump("plan", 65, 2048, 64) == dict(n=65, N=2048, tiles=1, ksplit=4, rows_per_chunk=512, slab_bytes=8 * 4 * 128 * 256, pairs=0, np2=0,
                                              issued=2.0 * 128 * 256 * 2048)
    assert dump("plan", 65, 2048, 0)["ksplit"] == 4                          # (nbatch < 1 counts as 1: 4096 asks for more than 4 allow)
    # the pair form: 47 tiles (test_tiles); 4096 / 47 asks for 88, ks in [44, 176]; 47 * 49 = 2303 = 9 * 256 - 1 is the fullest last round
    assert dump("plan_pairs", 100, 8, 100000) == dict(n=1600, N=100000, tiles=47, ksplit=49, rows_per_chunk=2048, slab_bytes=8 * 47 * 49 * 128 * 256,
                                                      pairs=36, np2=200, issued=47 * 2.0 * 128 * 256 * 49 * 2048)
    assert dump("plan_pairs", 8, 2, 600) == dict(n=32, N=600, tiles=1, ksplit=1, rows_per_chunk=640, slab_bytes=262144, pairs=3, np2=16,
                                                 issued=2.0 * 128 * 256 * 640)


KR_MODE, PANEL_MODE, KRS_MODE = 0, 1, 2


@pytest.mark.parametrize("mode,nb,ldk,stage", [
    # KR: (nfI + nfJ) frequencies x 16 B and ldk activations per sample, two images, 10240 doubles each at the most
    (KR_MODE, 8, 9, 32),          # 26 frequencies: 1664 + 384 doubles at 32 samples
    (KR_MODE, 1, 2, 16),          # 194 frequencies: 12416 doubles at 32, 6272 + 128 at 16
    (KR_MODE, 640, 641, 8),       # the activations: 10368 doubles at 16, 5248 + 128 at 8
    (KR_MODE, 1300, 1301, 0),     # 10496 doubles of activations at 8
    (KRS_MODE, 18, 171, 32),      # 68 frequencies: 4352 + 5504 doubles at 32
    (KRS_MODE, 19, 190, 16),      # 4352 + 6144 at 32; 2176 + 3072 at 16
    (KRS_MODE, 32, 528, 0),       # 2176 + 8448 at 16, and no instance at 8
    (PANEL_MODE, 0, 0, 16),       # the one panel instance
])
def test_stage_ladder(dump, mode, nb, ldk, stage):
    assert dump("stage", mode, nb, ldk)["stage"] == stage


def test_lds_bytes_and_the_pair_forms_limit(dump):
    assert dump("stage", KR_MODE, 8, 9) == dict(stage=32, lds32=16 * (1664 + 384), lds16=16 * (896 + 256), lds8=16 * (512 + 128))
    assert dump("stage", PANEL_MODE, 0, 0)["lds16"] == 16 * (16 * 384 + 128)   # 2 x 49 KiB
    # 16 samples per stage: 2176 doubles of trig values + 16 P of pair products <= 10240: P <= 504, nb (nb + 1) / 2 = 496 at nb = 31
    assert dump("krs_fits", 31)["fits"] == 1 and dump("krs_fits", 32)["fits"] == 0
    assert dump("krs_fits", 2)["fits"] == 1 and dump("krs_fits", 1)["fits"] == 0


def test_flop_counts(dump):
    assert dump("flops", 600, 12, 24, 3) == dict(gram=600.0 * 12 * 13, structured=8.0 * 600 * 24 * 3)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_sanitized_run_over_all_cases(dump, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan, stand-alone, once over every call the tests above made: it ends clean."""
    slots(dump, README_GRID); slots(dump, put(README_GRID, 7, NAN)); dump("plan", 1000, 100000, 1)   # (when this test runs alone)
    d, exe = _build(tmp_path_factory, "gram_form_plan_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    try:
        for argv in list(CALLS):
            r = subprocess.run([exe] + argv, capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", (argv, r.stderr[-2000:])
    finally:
        shutil.rmtree(d, ignore_errors=True)
