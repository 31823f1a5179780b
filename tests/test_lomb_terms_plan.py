"""The plan of lombscargle(..., nterms=K) (csrc/lomb_terms_plan.h): signals and accumulators per thread of the sums
kernel, the slabs of samples, the rows of partial sums, and the refusals.  The header has no HIP dependency: a tiny host program is built
against it as it is and prints what it decides; CPU only.  Every expected value is a literal worked from the rules:
  ts = the largest of {4, 2, 1} with 4K + 2K ts <= 48 accumulators, 1 for a single signal;
  slabs: lomb_tiling's rule -- about 2048 workgroups over (tiles of 64 frequencies x slabs), a slab never below 1024 samples, at most 1024
  slabs, the slab a multiple of 256 -- a function of N and Nf alone;
  rows = 4K + 2K ns."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: lomb_terms_plan_dump N Nf ns nterms
PROGRAM = r"""
#include "lomb_terms_plan.h"
#include <cstdio>
#include <cstdlib>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const LombTermsPlan p = lomb_terms_plan(atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), atoll(argv[4]));
    printf("status=%d K=%d ts=%d acc=%d sblocks=%d ftiles=%lld slab=%lld nslab=%lld rows=%lld part=%lld maxterms=%d\nwhy=%s\n", p.status, p.K, p.ts, p.acc, p.sblocks,
           (long long)p.ftiles, (long long)p.slab_samples, (long long)p.nslab, (long long)p.rows, (long long)p.part_doubles, kLombMaxTerms, p.why.c_str());
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
    """plan(N, Nf, ns, nterms) -> dict of the plan's fields and `why`."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("lomb_terms_plan")
    src, exe = os.path.join(d, "lomb_terms_plan_dump.cpp"), os.path.join(d, "lomb_terms_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-x", "c++", "-I", HEADER_DIR, src, "-o", exe])   # (host only: no HIP runtime)

    def run(N, Nf, ns, nterms):
        lines = subprocess.check_output([exe] + [str(v) for v in (N, Nf, ns, nterms)], text=True).split("\n")
        r = {k: int(v) for k, v in (item.split("=") for item in lines[0].split())}
        r["why"] = lines[1].split("=", 1)[1]
        return r
    return run


OK, ARGUMENT, UNSUPPORTED = 0, 1, 2
# K -> (signals per thread of a multi-signal call, accumulators of that thread)
TABLE = {1: (4, 12), 2: (4, 24), 3: (4, 36), 4: (4, 48), 5: (2, 40), 6: (2, 48)}


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_signals_and_accumulators_per_thread(plan, K):
    assert plan(1000, 70, 2, K)["maxterms"] == 6
    for ns in (1, 2, 5):
        r = plan(1000, 70, ns, K)
        ts, acc = (1, 6 * K) if ns == 1 else TABLE[K]
        assert r["status"] == OK and (r["K"], r["ts"], r["acc"]) == (K, ts, acc), (K, ns, r)
        assert r["acc"] <= 48 and r["sblocks"] == -(-ns // ts)
        assert r["rows"] == 4 * K + 2 * K * ns and r["part"] == r["nslab"] * r["rows"] * 70


@pytest.mark.parametrize("N,slab,nslab", [(1, 256, 1), (1000, 1024, 1), (2501, 1024, 3), (1 << 20, 1024, 1024)])
def test_the_slabs_depend_on_the_samples_and_frequencies_alone(plan, N, slab, nslab):
    for K in (1, 2, 6):
        for ns in (1, 2, 5):
            r = plan(N, 70, ns, K)
            assert (r["slab"], r["nslab"], r["ftiles"]) == (slab, nslab, 2), (K, ns, r)
    # 4096 frequencies are 64 tiles: 2048 / 64 = 32 slabs wanted
    want = {1: (256, 1), 1000: (1024, 1), 2501: (1024, 3), 1 << 20: (32768, 32)}[N]
    r = plan(N, 4096, 3, 4)
    assert (r["slab"], r["nslab"], r["ftiles"]) == (*want, 64)


def test_refusals_and_their_messages(plan):
    for K in (0, 7, -1, 100):
        r = plan(1000, 70, 2, K)
        assert r["status"] == ARGUMENT and r["why"] == f"lombscargle: nterms must be 1 .. 6, got {K}", r
    for args in ((0, 70, 1), (1000, 0, 1), (1000, 70, 0), (1000, 70, 65536), (-3, 70, 1)):
        r = plan(*args, 2)
        assert r["status"] == ARGUMENT and r["why"] == f"need N > 0, Nf > 0 and 1 <= ns <= 65535 (N = {args[0]}, Nf = {args[1]}, ns = {args[2]})", r
    assert plan(1000, 70, 65535, 2)["status"] == OK
    r = plan(1000, (1 << 24) + 1, 1, 2)
    assert r["status"] == UNSUPPORTED and r["why"] == f"{(1 << 24) + 1} frequencies are too many"
    assert plan(1000, 1 << 24, 1, 6)["status"] == OK
    # rows x Nf elements take a thread each in grids of 256: at most 255 (2^31 - 1) of them
    r = plan(1000, 1 << 24, 65535, 6)                                         # (24 + 12 x 65535) x 2^24 = 1.3e13
    assert r["status"] == UNSUPPORTED and "more than one call takes" in r["why"] and "nterms = 6" in r["why"] and "65535 signals" in r["why"]
    assert plan(1000, 1 << 24, 2000, 6)["status"] == OK                       # 24024 x 2^24 = 4.0e11 < 5.5e11
    assert plan(1000, 1 << 24, 2800, 6)["status"] == UNSUPPORTED              # 33624 x 2^24 = 5.6e11
