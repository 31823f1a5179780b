"""The plan of bls (csrc/bls_plan.h): the shifts of the quantisation, the frequencies a workgroup folds from one staged
block of samples (F), the signals of a pass (TS), the LDS bytes, the passes, the boxes tried, and every refusal with its message.  The
header has no HIP dependency: a tiny host program is built against it as it is and prints what it decides; CPU only.  Every expected
value is a literal worked from the rules:
  LDS = F nbins ((ts + weighted) 8 + 4) bytes, at most 63 KiB;
  ts = 1, 2 or 4 (the smallest that holds ns, at most 4), halved while one frequency does not fit;
  F = 4, halved while the histograms do not fit or fewer than 256 workgroups would be left;
  shy = 61 - ceil(log2 N) - (ilogb(A) + 1).
The same program is also built with -fsanitize=address,undefined and run over the same shapes (a stand-alone program with its own main)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: bls_plan_dump N ns nbins min_count unit normalization A f.. : kmin.. : kmax..
PROGRAM = r"""
#include "bls_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 8) return 2;
    const long long N = atoll(argv[1]), ns = atoll(argv[2]), nbins = atoll(argv[3]), min_count = atoll(argv[4]);
    const int unit = atoi(argv[5]), normalization = atoi(argv[6]);
    const double A = atof(argv[7]);
    std::vector<double> f;
    std::vector<int32_t> k[2];
    int which = 0;
    for (int i = 8; i < argc; ++i) {
        if (!strcmp(argv[i], ":")) { ++which; continue; }
        if (which == 0) f.push_back(atof(argv[i])); else k[which - 1].push_back(atoi(argv[i]));
    }
    long long Nf = (long long)f.size();
    if (getenv("BLS_NF")) {                                                    // (a long grid: the arrays filled with their first entries)
        Nf = atoll(getenv("BLS_NF"));
        if (Nf <= (1 << 24)) { f.resize((size_t)Nf, f[0]); k[0].resize((size_t)Nf, k[0][0]); k[1].resize((size_t)Nf, k[1][0]); }
    }
    const BlsPlan p = bls_plan(N, ns, f.data(), Nf, nbins, k[0].data(), k[1].data(), min_count, unit != 0, normalization);
    printf("status=%d F=%d ts=%d passes=%d unit=%d log2n=%d lds=%lld workgroups=%lld boxes=%.17g\nwhy=%s\n", p.status, p.F, p.ts, p.passes, p.unit, p.log2n,
           (long long)p.lds_bytes, (long long)p.workgroups, p.boxes, p.why.c_str());
    if (A > 0 && N >= 1) {
        const int sh = bls_shift_y(A, N);
        printf("shift=%d qmax=%lld qmin=%lld qw=%lld\n", sh, bls_quantise(A, sh), bls_quantise(-A, sh), bls_quantise(1.0 / (double)N, kBlsWeightShift));
        // the two words of YY for the terms A, A / 3, A / 7 (A the largest) and what they add up to
        const double v[3] = {A, A / 3.0, A / 7.0};
        long long hi = 0, lo = 0;
        for (double x : v) { long long h, l; bls_yy_words(x, sh, bls_log2_ceil(N), &h, &l); hi += h; lo += l; }
        printf("yyhi=%lld yylo=%lld yy=%.17g\n", hi, lo, bls_yy(hi, lo, sh, bls_log2_ceil(N)));
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
    src, exe = os.path.join(d, "bls_plan_dump.cpp"), os.path.join(d, "bls_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR] + flags + [src, "-o", exe])   # (host only: no HIP runtime)

    def run(N, ns, nbins, f=(1.0,), kmin=1, kmax=4, min_count=1, unit=False, normalization=0, A=0.0, env=None):
        f = list(np.atleast_1d(f))
        k0, k1 = np.broadcast_to(kmin, (len(f),)), np.broadcast_to(kmax, (len(f),))
        args = [N, ns, nbins, min_count, int(unit), normalization, repr(float(A))] + [repr(float(x)) for x in f] + [":"] + [int(x) for x in k0] + [":"] + [int(x) for x in k1]
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True, env=dict(os.environ, **(env or {})))
        r = {}
        for line in out.split("\n"):
            if line.startswith("why="):
                r["why"] = line[4:]
            elif line:
                for item in line.split():
                    k, v = item.split("=")
                    r[k] = float(v) if k in ("boxes", "yy") else int(v)
        return r
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build(tmp_path_factory, "bls_plan", ["-O1"])


OK, ARGUMENT, UNSUPPORTED = 0, 1, 2
# (N, Nf, nbins, ns, unit) -> (F, ts, LDS bytes, passes)
TABLE = [
    ((1500, 1, 64, 1, True), (1, 1, 768, 1)),
    ((1500, 70, 64, 1, True), (1, 1, 768, 1)),
    ((1500, 70, 100, 1, False), (1, 1, 2000, 1)),
    ((255, 70, 8, 3, False), (1, 4, 352, 1)),
    ((256, 70, 64, 5, True), (1, 4, 2304, 2)),
    ((1500, 70, 64, 2, False), (1, 2, 1792, 1)),
    ((1500, 1023, 64, 1, True), (4, 1, 3072, 1)),            # ceil(1023 / 4) = 256 workgroups: just enough
    ((1500, 1021, 64, 1, True), (4, 1, 3072, 1)),            # ceil(1021 / 4) = 256
    ((1500, 1020, 64, 1, True), (2, 1, 1536, 1)),            # ceil(1020 / 4) = 255 < 256, ceil(1020 / 2) = 510
    ((1500, 511, 64, 1, True), (2, 1, 1536, 1)),             # ceil(511 / 2) = 256
    ((1500, 510, 64, 1, True), (1, 1, 768, 1)),              # ceil(510 / 2) = 255 < 256
    ((1500, 1030, 64, 1, True), (4, 1, 3072, 1)),
    ((1500, 1030, 2048, 1, True), (2, 1, 49152, 1)),         # 4 x 2048 x 12 = 98304 > 64512
    ((1500, 1030, 2048, 1, False), (1, 1, 40960, 1)),        # 2 x 2048 x 20 = 81920 > 64512
    ((1500, 70, 2048, 3, False), (1, 2, 57344, 2)),          # one frequency of four signals: 2048 x 44 = 90112 > 64512; of two: 57344
    ((1500, 70, 2048, 5, True), (1, 2, 40960, 3)),           # unit weights: 2048 x (32 + 4) = 73728 > 64512; two signals: 2048 x 20
    ((1500, 1030, 8, 3, False), (4, 4, 1408, 1)),
    ((1 << 20, 65536, 512, 1, False), (4, 1, 40960, 1)),
    ((1 << 20, 65536, 1024, 1, False), (2, 1, 40960, 1)),    # 4 x 1024 x 20 = 81920 > 64512
    ((1 << 20, 65536, 128, 7, False), (4, 4, 22528, 2)),
]


def _expected(N, Nf, nbins, ns, unit):
    """The rules of the header, restated: what the literals of TABLE were worked from."""
    lds = lambda F, ts: F * nbins * ((ts + (0 if unit else 1)) * 8 + 4)     # noqa: E731
    ts = 1 if ns <= 1 else 2 if ns == 2 else 4
    while ts > 1 and lds(1, ts) > 63 * 1024:
        ts >>= 1
    F = 4
    while F > 1 and (lds(F, ts) > 63 * 1024 or -(-Nf // F) < 256):
        F >>= 1
    return F, ts, lds(F, ts), -(-ns // ts)


@pytest.mark.parametrize("shape,want", TABLE)
def test_frequencies_per_workgroup_signals_per_pass_lds_and_passes(plan, shape, want):
    N, Nf, nbins, ns, unit = shape
    assert _expected(*shape) == want, "the literal does not follow the stated rules"
    r = plan(N, ns, nbins, f=[1.0], kmin=1, kmax=nbins // 2, unit=unit, env={"BLS_NF": str(Nf)})
    assert r["status"] == OK and (r["F"], r["ts"], r["lds"], r["passes"]) == want, r
    assert r["lds"] <= 63 * 1024 and 2 * (r["lds"] + 1024) <= 160 * 1024                  # two workgroups per CU, whatever the shape
    assert r["workgroups"] == -(-Nf // r["F"]) and r["unit"] == int(unit) and r["log2n"] == int(np.ceil(np.log2(N)))
    assert r["boxes"] == float(Nf) * nbins * (nbins // 2)


def test_the_boxes_tried_follow_the_widths(plan):
    r = plan(1500, 1, 100, f=[1.0, 2.0, 3.0], kmin=[1, 2, 5], kmax=[1, 12, 50])
    assert r["status"] == OK and r["boxes"] == 100.0 * (1 + 11 + 46)


@pytest.mark.parametrize("N,A,shift", [(1500, 2.0 ** -10, 61 - 11 + 9), (1500, 1.5 * 2.0 ** -10, 59), (1 << 20, 1.0, 61 - 20 - 1), ((1 << 20) + 1, 1.0, 39),
                                       (1 << 24, 0.999, 61 - 24 - 0), (1, 3.0, 61 - 0 - 2), (255, 5e-324, 61 - 8 + 1073), (1 << 30, 1e300, 61 - 30 - 997)])
def test_the_shift_and_what_it_makes_of_the_largest_sample(plan, N, A, shift):
    r = plan(N, 1, 64, A=A)
    L = int(np.ceil(np.log2(N))) if N > 1 else 0
    assert r["shift"] == shift and r["log2n"] == L
    assert r["qmax"] == -r["qmin"] and 2 ** (60 - L) <= r["qmax"] <= 2 ** (61 - L)      # the largest sample uses the top bit the rule leaves it
    assert r["qmax"] * N <= 2 ** 61                                                     # ... and N of them stay inside 63 bits with room for S - s
    assert abs(r["qw"] * N - 2 ** 60) <= N / 2 + 2 ** 8                                 # the unit weight 1 / N: N of them make 2^60 up to the roundings


@pytest.mark.parametrize("N,A", [(3, 1.0), (1500, 0.37), (1 << 20, 1e-300), (1 << 30, 1e300), (255, 5e-324)])
def test_the_words_of_yy_add_up_to_the_sum_of_the_terms(plan, N, A):
    """YY is added up as two integer words per term (bls_yy_words) against the largest term: hi <= 2^(61 - L) each, the words of three terms
    give the sum of the terms to two roundings."""
    from fractions import Fraction
    r = plan(N, 1, 64, A=A)
    L = r["log2n"]
    exact = Fraction(A) + Fraction(A / 3.0) + Fraction(A / 7.0)
    assert 0 < r["yyhi"] <= 3 * 2 ** (61 - L) and abs(r["yylo"]) <= 3 * 2 ** (60 - L)
    assert abs(Fraction(r["yy"]) - exact) <= 2 * Fraction(2.0 ** -53) * exact + Fraction(5e-324)


def test_refusals_and_their_messages(plan):
    for N, ns, nf in ((0, 1, 2), (10, 0, 2), (10, 65536, 2), (10, 1, 0), (-1, 1, 2)):
        r = plan(N, ns, 64, f=[1.0, 2.0][:nf])
        assert r["status"] == ARGUMENT and r["why"] == f"bls: need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = {N}, Nf = {nf}, ns = {ns})", r
    assert plan(10, 65535, 64)["status"] == OK
    r = plan((1 << 30) + 1, 1, 64)
    assert r["status"] == UNSUPPORTED and r["why"] == f"bls: {(1 << 30) + 1} samples are more than 2^30"
    assert plan(1 << 30, 1, 64)["status"] == OK
    big = (1 << 24) + 1
    r = plan(10, 1, 64, env={"BLS_NF": str(big)})
    assert r["status"] == UNSUPPORTED and r["why"] == f"bls: {big} frequencies are more than 2^24"
    for nb in (7, 0, -3, 2049):
        r = plan(10, 1, nb)
        assert r["status"] == ARGUMENT and r["why"] == f"bls: nbins must lie in 8 .. 2048, got {nb}"
    assert plan(10, 1, 8)["status"] == OK and plan(10, 1, 2048)["status"] == OK
    for mc in (0, -1):
        assert plan(10, 1, 64, min_count=mc)["why"] == f"bls: min_count must be at least 1, got {mc}"
    for nm in (2, -1):
        assert plan(10, 1, 64, normalization=nm)["why"] == f"bls: normalization must be 0 (standard) or 1 (chi2), got {nm}"
    for bad in (np.nan, np.inf, -np.inf):
        r = plan(10, 1, 64, f=[1.0, bad])
        assert r["status"] == ARGUMENT and r["why"] == "bls: a frequency is not finite"
    for bad in (0.0, -0.5):
        assert plan(10, 1, 64, f=[1.0, bad])["why"] == "bls: frequency 1 is not positive"
    assert plan(10, 1, 64, f=[1.0, 2.0], kmin=[1, 0])["why"] == "bls: kmin of frequency 1 is 0, below 1"
    assert plan(10, 1, 64, f=[1.0, 2.0], kmin=[1, 9], kmax=[4, 8])["why"] == "bls: kmin of frequency 1 is 9, above its kmax 8"
    assert plan(10, 1, 64, f=[1.0, 2.0], kmin=1, kmax=[32, 33])["why"] == "bls: kmax of frequency 1 is 33, above nbins / 2 = 32"
    assert plan(10, 1, 9, kmin=1, kmax=5)["why"] == "bls: kmax of frequency 0 is 5, above nbins / 2 = 4"
    assert plan(10, 1, 64, kmin=32, kmax=32)["status"] == OK


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """A stand-alone host program with its own main, built with -fsanitize=address,undefined and run over the table's shapes, the shifts'
    extremes and every refusal: any report makes the program exit non-zero (-fno-sanitize-recover)."""
    run = _build(tmp_path_factory, "bls_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for (N, Nf, nbins, ns, unit), want in TABLE:
        r = run(N, ns, nbins, f=[1.0], kmin=1, kmax=nbins // 2, unit=unit, A=0.37, env={"BLS_NF": str(Nf)})
        assert (r["F"], r["ts"], r["lds"], r["passes"]) == want
    for N, A in ((1, 3.0), (255, 5e-324), (1 << 30, 1e300), (1 << 24, 0.999)):
        assert run(N, 1, 64, A=A)["status"] == OK
    assert run(0, 1, 64)["status"] == ARGUMENT and run(10, 1, 64, f=[1.0, np.nan])["status"] == ARGUMENT
    assert run(10, 1, 64, f=[1.0, 2.0], kmin=[1, 9], kmax=[4, 8])["status"] == ARGUMENT and run(10, 1, 5000)["status"] == ARGUMENT
    assert run(10, 1, 64, env={"BLS_NF": str((1 << 24) + 1)})["status"] == UNSUPPORTED
