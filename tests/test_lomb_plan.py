"""What lombscargle decides on the host before anything is launched (csrc/lomb_plan.h): the admission of a frequency
grid to the transform path, the cut of a long grid into blocks of modes, the real weight vectors of a block's transforms, the signal
groups, the path `auto` takes, the direct path's tiling and the slabs of the fixed-order sums.  The header has no HIP dependency: a
tiny host program is built against it as it is and prints what it decides; CPU only.  Every expected value is a literal worked from the
rules.

    1  admission: progressions from 0, from D and from an arbitrary a; a perturbed grid; residuals just under and over the phase limit
    2  blocks at Nf = 1, 2100, 2101, 4200, 4201 and with the knob at 64; bases, pre-phase flags, residuals inside a block, fine grids
    3  weight vectors with and without the pre-phase; signal groups at ns = 127, 128
    4  the path on both sides of each of its thresholds and for explicit requests
    5  tiling and slabs of the direct path"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: lomb_plan_dump MODE ARGUMENT ...  ->  one line of key=value pairs; doubles go in and out as hexadecimal floats (%a)
PROGRAM = r"""
#include "lomb_plan.h"
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
    if (mode == "admit") {                // tam f ...
        if (d.size() < 2) return 2;
        const LombGrid g = lomb_admit(std::vector<double>(d.begin() + 1, d.end()), d[0]);
        printf("ok=%d twin=%d emax=%a a=%a D=%a w1_hi=%a w1_lo=%a w2_hi=%a w2_lo=%a\n", (int)g.ok, (int)g.twin, g.emax, g.a, g.D, g.w1_hi, g.w1_lo, g.w2_hi, g.w2_lo);
    } else if (mode == "blocks") {        // Nf knob a D: the grid a + k D
        if (d.size() != 4) return 2;
        std::vector<double> f((size_t)v[0]);
        for (size_t k = 0; k < f.size(); ++k) f[k] = d[2] + (double)k * d[3];
        const int L = lomb_block_len(v[1]);
        const std::vector<LombBlock> bl = lomb_blocks(f, L);
        printf("L=%d max=%d nblocks=%d nf=%d k0=", L, lomb_max_block(), (int)bl.size(), lomb_fine_grid((long long)f.size(), L));
        for (size_t b = 0; b < bl.size(); ++b) printf(b ? ",%lld" : "%lld", (long long)bl[b].k0);
        printf(" count=");
        for (size_t b = 0; b < bl.size(); ++b) printf(b ? ",%d" : "%d", bl[b].count);
        printf(" base=");
        for (size_t b = 0; b < bl.size(); ++b) printf(b ? ",%a" : "%a", bl[b].base);
        printf(" prephase=");
        for (size_t b = 0; b < bl.size(); ++b) printf(b ? ",%d" : "%d", (int)bl[b].prephase);
        printf("\n");
    } else if (mode == "residuals") {     // L f ...: eps' of every frequency against its block
        if (d.size() < 3) return 2;
        const std::vector<double> f(d.begin() + 1, d.end());
        const LombGrid g = lomb_admit(f, 1.0);
        const std::vector<double> e = lomb_block_residuals(f, g, (int)v[0]);
        printf("ok=%d eps=", (int)g.ok);
        for (size_t k = 0; k < e.size(); ++k) printf(k ? ",%a" : "%a", e[k]);
        printf("\n");
    } else if (mode == "weights") {       // family g prephase
        need(3);
        printf("nq=%d\n", lomb_weight_vectors((int)v[0], (int)v[1], v[2] != 0));
    } else if (mode == "groups") {        // ns
        need(1);
        printf("groups=%lld per=%d max=%lld\n", (long long)lomb_signal_groups(v[0]), kLombGroupSignals, (long long)kNufftMaxWeights);
    } else if (mode == "path") {          // requested grid_ok N Nf
        need(4);
        printf("path=%d samples=%lld freqs=%lld work=%lld\n", lomb_choose_path((int)v[0], v[1] != 0, v[2], v[3]), (long long)kLombNufftMinSamples,
               (long long)kLombNufftMinFreqs, (long long)kLombNufftMinWork);
    } else if (mode == "needs") {         // requested N Nf
        need(3);
        printf("needs=%d\n", (int)lomb_needs_admission((int)v[0], v[1], v[2]));
    } else if (mode == "yynoise") {       // N center fit_mean R YY
        if (d.size() != 5) return 2;
        printf("emax=%a\n", lomb_yy_noise(d[0], v[1] != 0, v[2] != 0, d[3], d[4]));
    } else if (mode == "tiling") {        // N Nf ns
        need(3);
        const LombTiling t = lomb_tiling(v[0], v[1], v[2]);
        printf("ts=%d sblocks=%d acc=%d ftiles=%lld slab=%lld nslab=%lld sums=%lld\n", t.ts, t.sblocks, t.acc, (long long)t.ftiles, (long long)t.slab_samples,
               (long long)t.nslab, (long long)lomb_sum_slabs(v[0]));
    } else return 2;
    return 0;
}
"""

DOUBLES = ("emax", "a", "D", "w1_hi", "w1_lo", "w2_hi", "w2_lo")
LISTS_F = ("eps", "base")
LISTS_I = ("k0", "count", "prephase")


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
        elif k in LISTS_F:
            r[k] = [float.fromhex(x) for x in v.split(",") if x]
        elif k in LISTS_I:
            r[k] = [int(x) for x in v.split(",") if x]
        else:
            r[k] = int(v)
    return r


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(mode, arguments...) -> the dict the program prints."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("lomb_plan")
    src, exe = os.path.join(d, "lomb_plan_dump.cpp"), os.path.join(d, "lomb_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(mode, *args):
        return _parse(subprocess.check_output([exe, mode] + [_arg(a) for a in args], text=True))
    return run


PI_Q = Fraction("3.1415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679")
TINY = Fraction(1, 2 ** 100)


# ---- 1  admission ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0.0, 0.5, 37.25 * 0.5])                 # from 0, from D and from an arbitrary a = 37.25 D
def test_progressions_are_admitted_with_their_angular_steps_in_double_double(dump, first):
    """Binary fractions, so the step in cycles is exact: hi + lo is 2 pi D to 2^-100 of it (a 100-digit pi in rational arithmetic)."""
    r = dump("admit", 100.0, *[first + 0.5 * k for k in range(8)])
    assert (r["ok"], r["twin"], r["emax"], r["a"], r["D"]) == (1, 0, 0.0, first, 0.5)
    assert abs(Fraction(r["w1_hi"]) + Fraction(r["w1_lo"]) - PI_Q) <= TINY * PI_Q
    assert abs(Fraction(r["w2_hi"]) + Fraction(r["w2_lo"]) - 2 * PI_Q) <= TINY * 2 * PI_Q
    assert r["w1_hi"] == np.pi and r["w2_hi"] == 2 * np.pi and abs(r["w1_lo"]) <= 2.0 ** -53 * np.pi and r["w1_lo"] != 0.0


@pytest.mark.parametrize("first", [0.0, 37.25])
@pytest.mark.parametrize("L", [200, 64])
def test_steps_and_block_residuals_hold_the_real_frequencies_late_in_a_record(dump, first, L):
    """A grid whose step is no binary fraction, up to f = 2.9, at t = 2^20: mode j of a block stands for base + j D + eps'_j.  In rational
    arithmetic, |j (w1_hi + w1_lo) + 2 pi eps'_j - 2 pi (f[k0 + j] - f[k0])| 2^20 is what the plan itself puts between the transform and
    the real phase.  Worked in long double it was 1.0e-12 rad in one block of 200 (family 2: twice that) against the 1e-12 the
    transforms are held to; in double-double the rounding of the residuals to doubles is left."""
    D = 0.0123
    f = [first * D + D * k for k in range(200)]
    g = dump("admit", 2.0 ** 20, *f)
    e = dump("residuals", L, *f)["eps"]
    assert g["ok"] == 1 and g["twin"] == 1 and len(e) == 200
    w1, w2 = Fraction(g["w1_hi"]) + Fraction(g["w1_lo"]), Fraction(g["w2_hi"]) + Fraction(g["w2_lo"])
    worst = Fraction(0)
    for k in range(200):
        k0 = k // L * L
        true = 2 * PI_Q * (Fraction(f[k]) - Fraction(f[k0]))
        worst = max(worst, abs((k - k0) * w1 + 2 * PI_Q * Fraction(e[k]) - true), abs((k - k0) * w2 + 4 * PI_Q * Fraction(e[k]) - 2 * true) / 2)
    print(f"a = {first} D, blocks of {L}: the plan's own phase error {float(worst * 2 ** 20):.3e} rad")
    assert worst * 2 ** 20 <= Fraction(1, 10 ** 20)


def test_perturbed_grid_is_refused(dump):
    f = [0.5 * k for k in range(8)]
    f[2] += 1e-3
    r = dump("admit", 100.0, *f)
    assert r["ok"] == 0 and r["emax"] == f[2] - 1.0


@pytest.mark.parametrize("tam,admitted", [(17.0, 1), (18.0, 0)])
def test_residual_phase_on_both_sides_of_the_limit(dump, tam, admitted):
    """One residual of 2^-30 (the end points fix a and D): its phase 2 pi 2^-30 max|t| is 9.948e-8 at 17 and 1.0533e-7 at 18, against
    kApMaxResidualPhase = 1e-7.  Admitted grids with a residual take the first-order term."""
    f = [0.5 * k for k in range(8)]
    f[2] += 2.0 ** -30
    r = dump("admit", tam, *f)
    assert r["emax"] == 2.0 ** -30 and (r["ok"], r["twin"]) == (admitted, admitted)


def test_one_frequency_or_a_zero_step_is_no_progression(dump):
    assert dump("admit", 1.0, 0.7)["ok"] == 0
    assert dump("admit", 1.0, 0.7, 0.7, 0.7)["ok"] == 0
    assert dump("admit", float("inf"), 0.5, 1.0, 1.5)["ok"] == 0


# ---- 2  blocks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nf,k0,count,nf", [
    (1, [0], [1], 256),
    (2100, [0], [2100], 8192),                                             # 3.9 * 2100 = 8190 <= 8192: the longest block
    (2101, [0, 2100], [2100, 1], 8192),
    (4200, [0, 2100], [2100, 2100], 8192),
    (4201, [0, 2100, 4200], [2100, 2100, 1], 8192),
])
def test_block_counts_and_bases_of_a_grid_from_zero(dump, Nf, k0, count, nf):
    r = dump("blocks", Nf, 0, 0.0, 0.25)
    assert (r["L"], r["max"], r["nblocks"], r["nf"]) == (2100, 2100, len(k0), nf)
    assert r["k0"] == k0 and r["count"] == count
    assert r["base"] == [0.25 * k for k in k0] and r["prephase"] == [int(k > 0) for k in k0]   # a block from 0 needs no pre-phase


def test_blocks_from_a_nonzero_first_frequency_all_take_the_pre_phase(dump):
    r = dump("blocks", 2101, 0, 0.25, 0.25)
    assert r["base"] == [0.25, 525.25] and r["prephase"] == [1, 1]
    r = dump("blocks", 200, 0, 37.25 * 0.25, 0.25)
    assert r["nblocks"] == 1 and r["base"] == [9.3125] and r["prephase"] == [1] and r["nf"] == 1024   # 3.9 * 200 = 780


def test_the_knob_shortens_the_blocks(dump):
    r = dump("blocks", 200, 64, 0.0, 0.25)
    assert (r["L"], r["nblocks"], r["nf"]) == (64, 4, 256)                # 3.9 * 64 = 249.6
    assert r["k0"] == [0, 64, 128, 192] and r["count"] == [64, 64, 64, 8] and r["base"] == [0.0, 16.0, 32.0, 48.0] and r["prephase"] == [0, 1, 1, 1]
    assert dump("blocks", 200, 5000, 0.0, 0.25)["L"] == 2100 and dump("blocks", 200, -3, 0.0, 0.25)["L"] == 2100   # out of range: ignored
    assert dump("blocks", 200, 65, 0.0, 0.25)["nf"] == 256 and dump("blocks", 200, 66, 0.0, 0.25)["nf"] == 512


def test_residuals_are_taken_against_the_blocks_own_base(dump):
    """f = k/2 with f[5] moved by 2^-31 (blocks of 4: 5 is the second frequency of block 1) and f[4], a base, moved by 2^-32: the base is
    the frequency itself, so what its block's other frequencies miss is their own residual minus the base's."""
    f = [0.5 * k for k in range(8)]
    f[5] += 2.0 ** -31
    f[4] += 2.0 ** -32
    r = dump("residuals", 4, *f)
    assert r["ok"] == 1
    assert r["eps"] == [0.0, 0.0, 0.0, 0.0, 0.0, 2.0 ** -31 - 2.0 ** -32, -2.0 ** -32, -2.0 ** -32]


# ---- 3  weight vectors and signal groups -------------------------------------------------------------------------------------------------
def test_weight_vectors_with_and_without_the_pre_phase(dump):
    assert dump("weights", 1, 1, 0)["nq"] == 2 and dump("weights", 1, 1, 1)["nq"] == 4       # w and w y; twice with complex weights
    assert dump("weights", 1, 3, 0)["nq"] == 4 and dump("weights", 1, 3, 1)["nq"] == 8
    assert dump("weights", 2, 0, 0)["nq"] == 1 and dump("weights", 2, 0, 1)["nq"] == 2       # family 2: w alone
    assert dump("weights", 1, 127, 1)["nq"] == 256                                            # a full group fills kNufftMaxWeights


def test_signal_groups(dump):
    assert dump("groups", 127) == dict(groups=1, per=127, max=256)
    assert dump("groups", 128)["groups"] == 2 and dump("groups", 1)["groups"] == 1 and dump("groups", 255)["groups"] == 3


# ---- 4  the path ---------------------------------------------------------------------------------------------------------------------------
def test_auto_takes_the_transforms_on_the_far_side_of_its_three_thresholds(dump):
    """Measured constants (profiles/lomb_time.txt): 2^18 samples -- not the structured Gram's 4096 --, 512 frequencies, N Nf = 2^29."""
    r = dump("path", 0, 1, 1 << 18, 2048)
    assert r == dict(path=2, samples=1 << 18, freqs=512, work=1 << 29)
    assert dump("path", 0, 1, (1 << 18) - 1, 1 << 16)["path"] == 1         # one sample short, whatever the grid
    assert dump("path", 0, 1, 1 << 22, 511)["path"] == 1 and dump("path", 0, 1, 1 << 20, 512)["path"] == 2   # one frequency short
    assert dump("path", 0, 1, 1 << 18, 2047)["path"] == 1 and dump("path", 0, 1, 1 << 19, 1024)["path"] == 2   # the work on both sides of 2^29
    assert dump("path", 0, 1, 1 << 19, 1023)["path"] == 1
    assert dump("path", 0, 0, 1 << 20, 4096)["path"] == 1                  # a grid that is not admitted: direct at any size


def test_explicit_paths(dump):
    assert dump("path", 1, 1, 1 << 20, 4096)["path"] == 1
    assert dump("path", 2, 1, 1, 1)["path"] == 2                           # asked for: no thresholds
    assert dump("path", 2, 0, 1 << 20, 4096)["path"] == -1                 # refused
    assert dump("path", 3, 1, 1 << 20, 4096)["path"] == -1 and dump("path", -1, 1, 1 << 20, 4096)["path"] == -1


def test_the_grid_is_looked_at_only_when_the_transforms_can_be_taken(dump):
    assert dump("needs", 2, 10, 3)["needs"] == 1                           # asked for
    assert dump("needs", 1, 1 << 20, 4096)["needs"] == 0                   # direct: never
    assert dump("needs", 0, 1 << 18, 2048)["needs"] == 1 and dump("needs", 0, 1 << 18, 2047)["needs"] == 0 and dump("needs", 0, 4096, 512)["needs"] == 0


def test_what_counts_as_a_zero_signal_power(dump):
    """u = (N + 16) 2^-53 at N = 48 is 2^-47: centred u^2 R, fit_mean 3 u YY, both added, neither 0."""
    assert dump("yynoise", 48.0, 1, 0, 4.0, 1.0)["emax"] == 2.0 ** -92
    assert dump("yynoise", 48.0, 0, 1, 4.0, 1.0)["emax"] == 3 * 2.0 ** -47
    assert dump("yynoise", 48.0, 1, 1, 4.0, 1.0)["emax"] == 2.0 ** -92 + 3 * 2.0 ** -47
    assert dump("yynoise", 48.0, 0, 0, 4.0, 1.0)["emax"] == 0.0


# ---- 5  the direct path's tiling and the slabs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Nf,ns,want", [
    (1, 1, 1, dict(ts=1, sblocks=1, acc=6, ftiles=1, slab=256, nslab=1, sums=1)),
    (4097, 65, 3, dict(ts=4, sblocks=1, acc=12, ftiles=2, slab=1024, nslab=5, sums=17)),    # 5 slabs wanted of ceil(4097 / 5) = 820 -> 1024
    (1000, 7, 1, dict(ts=1, sblocks=1, acc=6, ftiles=1, slab=1024, nslab=1, sums=4)),
    (1 << 20, 512, 1, dict(ts=1, sblocks=1, acc=6, ftiles=8, slab=4096, nslab=256, sums=4096)),   # 8 tiles x 256 slabs = 2048 workgroups
    (1 << 20, 65536, 9, dict(ts=4, sblocks=3, acc=12, ftiles=1024, slab=524288, nslab=2, sums=4096)),
    (1 << 20, 1, 1, dict(ts=1, sblocks=1, acc=6, ftiles=1, slab=1024, nslab=1024, sums=4096)),    # at most 1024 slabs, never below 1024 samples
])
def test_direct_tiling_and_slabs(dump, N, Nf, ns, want):
    assert dump("tiling", N, Nf, ns) == want


def test_the_slabs_do_not_depend_on_the_number_of_signals(dump):
    a, b = dump("tiling", 4097, 65, 1), dump("tiling", 4097, 65, 3)
    assert (a["slab"], a["nslab"], a["ftiles"]) == (b["slab"], b["nslab"], b["ftiles"])
