"""The plan of wwz (csrc/wwz_plan.h): the decay per frequency, the sort of the times into groups of TT adjacent values,
times and signals per thread of the sums kernel, the tiles of frequencies, the slab length, the samples a (group, tile) stages, the work
list, the partial sums, staged against useful triples, and every refusal with its message.  The header has no HIP dependency: a tiny host
program is built against it as it is and prints what it decides; CPU only.  Every expected value is a literal worked from the rules:
  accumulators of a thread = TT (6 + 4 ts) <= 48: one signal ts = 1, TT = 4 (40); several ts = 4, TT = 2 (44); TT halved while half of
  it holds the whole list of times;
  slab = max(1024, ceil(N / 64) rounded up to 256): a function of N alone, at absolute multiples;
  a (group, tile) stages [#{t < gmin - rmax}, #{t <= gmax + rmax}) and leaves one item per slab that range touches."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: wwz_plan_dump N ns c max_items useful f.. : tau.. : radius.. : edges..     (edges may be absent: the shape alone)
PROGRAM = r"""
#include "wwz_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const long long N = atoll(argv[1]), ns = atoll(argv[2]);
    const double c = atof(argv[3]);
    const long long max_items = atoll(argv[4]);
    const double useful = atof(argv[5]);
    std::vector<double> v[3];
    std::vector<int64_t> edges;
    int which = 0;
    for (int i = 6; i < argc; ++i) {
        if (!strcmp(argv[i], ":")) { ++which; continue; }
        if (which < 3) v[which].push_back(atof(argv[i])); else edges.push_back(atoll(argv[i]));
    }
    long long Nf = (long long)v[0].size(), Ntau = (long long)v[1].size();
    if (getenv("WWZ_NF")) Nf = atoll(getenv("WWZ_NF"));                       // (counts beyond the arrays: refused before an array is read)
    if (getenv("WWZ_NTAU")) Ntau = atoll(getenv("WWZ_NTAU"));
    const WwzShape p = wwz_shape(N, ns, v[0].data(), Nf, v[1].data(), Ntau, c, v[2].data());
    printf("status=%d TT=%d ts=%d acc=%d sblocks=%d ngroups=%lld ftiles=%lld slab=%lld rows=%lld\nwhy=%s\n", p.status, p.TT, p.ts, p.acc, p.sblocks,
           (long long)p.ngroups, (long long)p.ftiles, (long long)p.slab_samples, (long long)p.rows, p.why.c_str());
    auto dumpd = [](const char *name, const std::vector<double> &a) { printf("%s=", name); for (double x : a) printf("%.17g,", x); printf("\n"); };
    auto dumpi = [](const char *name, const std::vector<int32_t> &a) { printf("%s=", name); for (int x : a) printf("%d,", x); printf("\n"); };
    dumpd("decay", p.decay); dumpi("order", p.order); dumpi("pos", p.pos); dumpd("tau", p.tau_sorted); dumpd("gmin", p.gmin); dumpd("gmax", p.gmax);
    dumpd("rmax", p.rmax);
    if (p.status != kWwzOk || edges.empty()) return 0;
    const WwzWork w = wwz_work(p, edges, useful, max_items > 0 ? max_items : kLombMaxGrid);
    printf("wstatus=%d part=%lld bytes=%.17g staged=%.17g useful=%.17g\nwwhy=%s\nitems=", w.status, (long long)w.part_doubles, w.part_bytes, w.staged, w.useful,
           w.why.c_str());
    for (const WwzItem &it : w.items) printf("%d/%d/%lld/%lld,", it.group, it.tile, (long long)it.first, (long long)it.last);
    printf("\noffset="); for (int64_t x : w.offset) printf("%lld,", (long long)x);
    printf("\nfirst_slab="); for (int64_t x : w.first_slab) printf("%lld,", (long long)x);
    printf("\n");
    return 0;
}
"""


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(N, ns, c, f, tau, radius, edges=(), useful=0, max_items=0, env=None) -> dict of what the program printed."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("wwz_plan")
    src, exe = os.path.join(d, "wwz_plan_dump.cpp"), os.path.join(d, "wwz_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(N, ns, c, f, tau, radius, edges=(), useful=0, max_items=0, env=None):
        args = [N, ns, repr(float(c)), max_items, repr(float(useful))] + [repr(float(x)) for x in f] + [":"] + [repr(float(x)) for x in tau] + [":"] + \
               [repr(float(x)) for x in radius] + [":"] + [int(x) for x in edges]
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True, env=dict(os.environ, **(env or {})))
        r = {}
        for line in out.split("\n"):
            if not line:
                continue
            if line.startswith(("why=", "wwhy=")):
                k, v = line.split("=", 1)
                r[k] = v
            elif line.startswith(("status=", "wstatus=")):
                for item in line.split():
                    k, v = item.split("=")
                    r[k] = float(v) if k in ("bytes", "staged", "useful") else int(v)
            else:
                k, v = line.split("=", 1)
                vals = [x for x in v.split(",") if x]
                r[k] = [tuple(int(q) for q in x.split("/")) for x in vals] if k == "items" else [float(x) for x in vals]
        return r
    return run


OK, ARGUMENT, UNSUPPORTED = 0, 1, 2
C0 = 1.0 / (8.0 * np.pi ** 2)


@pytest.mark.parametrize("ns,Ntau,TT,ts,acc,sblocks", [(1, 9, 4, 1, 40, 1), (1, 1, 1, 1, 10, 1), (1, 2, 2, 1, 20, 1), (1, 3, 4, 1, 40, 1), (1, 4, 4, 1, 40, 1),
                                                      (3, 9, 2, 4, 44, 1), (5, 9, 2, 4, 44, 2), (5, 1, 1, 4, 22, 2), (2, 2, 2, 4, 44, 1)])
def test_times_and_signals_per_thread(plan, ns, Ntau, TT, ts, acc, sblocks):
    r = plan(1500, ns, C0, [1.0, 2.0], np.arange(Ntau), [1.0, 0.5])
    assert r["status"] == OK and (r["TT"], r["ts"], r["acc"], r["sblocks"]) == (TT, ts, acc, sblocks), r
    assert r["acc"] <= 48 and r["rows"] == 6 + 4 * ns and r["ngroups"] == -(-Ntau // TT) and r["ftiles"] == 1


@pytest.mark.parametrize("N,slab", [(1, 1024), (1500, 1024), (3000, 1024), (65536, 1024), (65537, 1280), (1 << 17, 2048), (1 << 20, 16384), ((1 << 20) + 1, 16640)])
def test_the_slab_depends_on_the_samples_alone(plan, N, slab):
    for ns, taus in ((1, [0.0]), (1, np.arange(9)), (5, np.arange(3))):
        assert plan(N, ns, C0, np.arange(1, 71) / 8, taus, np.ones(70))["slab"] == slab


def test_the_decay_is_the_stated_double(plan):
    f = np.array([0.25, 1.015625, 3.0])
    for c in (C0, 1.0 / (512.0 * np.pi ** 2), 0.3):
        w = 6.283185307179586 * f
        assert plan(100, 1, c, f, [0.0], [1.0, 1.0, 1.0])["decay"] == list(c * (w * w))


def test_times_are_sorted_into_groups_and_outputs_keep_their_place(plan):
    r = plan(1500, 1, C0, [1.0], [5.0, 1.0, 3.0, 1.0, 9.0], [2.0])
    assert (r["TT"], r["ngroups"]) == (4, 2)
    assert r["order"] == [1, 3, 2, 0, 4]                                        # ties keep the caller's order
    assert r["pos"] == [3, 0, 2, 1, 4]
    assert r["tau"] == [1.0, 1.0, 3.0, 5.0, 9.0, 9.0, 9.0, 9.0]                 # the last group is padded with the largest time
    assert r["gmin"] == [1.0, 9.0] and r["gmax"] == [5.0, 9.0]
    r = plan(1500, 3, C0, [1.0], [5.0, 1.0, 3.0, 1.0, 9.0], [2.0])             # several signals: groups of two
    assert (r["TT"], r["ngroups"]) == (2, 3) and r["tau"] == [1.0, 1.0, 3.0, 5.0, 9.0, 9.0] and r["gmin"] == [1.0, 3.0, 9.0] and r["gmax"] == [1.0, 5.0, 9.0]


def test_a_tile_stages_its_largest_radius(plan):
    f = np.arange(1, 71) / 4.0                                                  # 70 frequencies: tiles of 64 and 6
    r = plan(1500, 1, C0, f, [0.0], 8.0 / f)
    assert r["ftiles"] == 2 and r["rmax"] == [32.0, 8.0 / (65 / 4.0)]
    r = plan(1500, 1, C0, f, [0.0], np.full(70, np.inf))
    assert r["rmax"] == [np.inf, np.inf]


def test_the_work_list(plan):
    """3000 samples, slab 1024, one group of 4 times x two tiles: the first pair reaches the samples [100, 2500) -- slabs 0, 1, 2 --,
    the second [1024, 1024): nothing."""
    f = np.arange(1, 71) / 4.0
    r = plan(3000, 1, C0, f, [0.0, 1.0, 2.0, 3.0], 8.0 / f, edges=[100, 2500, 1024, 1024], useful=12345.0)
    assert r["wstatus"] == OK and r["items"] == [(0, 0, 100, 1024), (0, 0, 1024, 2048), (0, 0, 2048, 2500)]
    assert r["offset"] == [0, 3, 3] and r["first_slab"] == [0, 1]
    assert r["part"] == 3 * 10 * 4 * 64 and r["bytes"] == 8.0 * r["part"]
    assert r["staged"] == 2400 * 64 * 4 and r["useful"] == 12345.0
    # a range that ends on a slab's edge leaves no empty item; one inside a single slab leaves one; five signals: 26 rows, groups of two
    r = plan(3000, 5, C0, f, [0.0, 1.0, 2.0, 3.0], 8.0 / f, edges=[0, 2048, 1030, 1040, 2047, 2049, 3000, 3000])
    assert r["items"] == [(0, 0, 0, 1024), (0, 0, 1024, 2048), (0, 1, 1030, 1040), (1, 0, 2047, 2048), (1, 0, 2048, 2049)]
    assert r["offset"] == [0, 2, 3, 5, 5] and r["first_slab"] == [0, 1, 1, 2]
    assert r["part"] == 5 * 26 * 2 * 64 and r["staged"] == (2048 + 10 + 2) * 64 * 2
    # the whole record of the wide case: 3000 samples cross the slab twice
    r = plan(3000, 1, C0, [1.0], [0.0], [np.inf], edges=[0, 3000])
    assert r["items"] == [(0, 0, 0, 1024), (0, 0, 1024, 2048), (0, 0, 2048, 3000)]


def test_refusals_and_their_messages(plan):
    f, tau, rad = [1.0, 2.0], [0.0, 1.0], [1.0, 1.0]
    for N, ns, nf, nt in ((0, 1, 2, 2), (10, 0, 2, 2), (10, 65536, 2, 2), (10, 1, 0, 2), (10, 1, 2, 0), (-1, 1, 2, 2)):
        r = plan(N, ns, C0, f[:nf], tau[:nt], rad[:nf])
        assert r["status"] == ARGUMENT and r["why"] == f"wwz: need N > 0, Nf > 0, Ntau > 0 and 1 <= ns <= 65535 (N = {N}, Nf = {nf}, Ntau = {nt}, ns = {ns})", r
    assert plan(10, 65535, C0, f, tau, rad)["status"] == OK
    big = (1 << 24) + 1
    r = plan(10, 1, C0, f, tau, rad, env={"WWZ_NF": str(big)})
    assert r["status"] == UNSUPPORTED and r["why"] == f"wwz: {big} frequencies are more than 2^24"
    r = plan(10, 1, C0, f, tau, rad, env={"WWZ_NTAU": str(big)})
    assert r["status"] == UNSUPPORTED and r["why"] == f"wwz: {big} times are more than 2^24"
    for c in (0.0, -1.0, np.nan, np.inf):
        r = plan(10, 1, c, f, tau, rad)
        assert r["status"] == ARGUMENT and r["why"] == "wwz: the decay c must be positive and finite"
    for bad in (np.nan, np.inf, -np.inf):
        assert plan(10, 1, C0, [1.0, bad], tau, rad)["why"] == "wwz: a frequency is not finite"
        assert plan(10, 1, C0, f, [bad, 0.0], rad)["why"] == "wwz: a time tau is not finite"
    for bad in (0.0, -0.5):
        r = plan(10, 1, C0, [1.0, bad], tau, rad)
        assert r["status"] == ARGUMENT and r["why"] == "wwz: frequency 1 is not positive"
    for bad in (0.0, -1.0, np.nan, -np.inf):
        r = plan(10, 1, C0, f, tau, [bad, 1.0])
        assert r["status"] == ARGUMENT and r["why"] == "wwz: radius 0 is not positive (or not a number)"
    assert plan(10, 1, C0, f, tau, [np.inf, 1.0])["status"] == OK
    # a work list longer than one launch takes (the limit is 2^31 - 1; a smaller one is handed in here)
    r = plan(3000, 1, C0, [1.0], [0.0], [np.inf], edges=[0, 3000], max_items=2)
    assert r["wstatus"] == UNSUPPORTED and r["wwhy"] == ("wwz: the work list (one item per group of times, tile of frequencies and slab of 1024 samples) has "
                                                        "3 items, more than the 2 one launch takes")
    assert plan(3000, 1, C0, [1.0], [0.0], [np.inf], edges=[0, 3000], max_items=3)["wstatus"] == OK
