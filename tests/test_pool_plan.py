"""The two pure decisions of the caching device allocator (csrc/pool_plan.h): which cached block answers a request -- the
smallest one of at least n bytes and at most n + n / 4 + 1 MiB -- and what the experiment knob LPVS_POOL_FILL asks for (exactly two
hexadecimal digits; anything else is off).  The header has no HIP dependency: a tiny host program is built against it as it is and prints
what it decides; CPU only.  The same program is also built with -fsanitize=address,undefined and run over the same cases (a stand-alone
program with its own main)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

# usage: pool_plan_dump fit n size..   -> "fit=<index of the block taken, in the order given, or -1> size=<its size or 0>"
#        pool_plan_dump parse [string] -> "fill=<byte or -1>"   (no string: a null pointer)
#        pool_plan_dump round n        -> "round=<bytes> slack=<bytes>"
PROGRAM = r"""
#include "pool_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace lpvs;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "fit")) {
        if (argc < 3) return 2;
        const size_t n = (size_t)strtoull(argv[2], nullptr, 10);
        std::multimap<size_t, int> cache;
        for (int i = 3; i < argc; ++i) cache.emplace((size_t)strtoull(argv[i], nullptr, 10), i - 3);
        auto it = pool_best_fit(cache, n);
        if (it == cache.end()) printf("fit=-1 size=0\n");
        else printf("fit=%d size=%zu\n", it->second, it->first);
        return 0;
    }
    if (!strcmp(argv[1], "parse")) { printf("fill=%d\n", pool_fill_parse(argc > 2 ? argv[2] : nullptr)); return 0; }
    if (!strcmp(argv[1], "round")) { printf("round=%zu slack=%zu\n", pool_round((size_t)strtoull(argv[2], nullptr, 10)), kPoolFillSlack); return 0; }
    return 2;
}
"""

MIB = 1 << 20


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
    src, exe = os.path.join(d, "pool_plan_dump.cpp"), os.path.join(d, "pool_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", HEADER_DIR] + flags + [src, "-o", exe])   # (host only: no HIP runtime)

    def run(*args):
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True)
        return {k: int(v) for k, v in (item.split("=") for item in out.split())}
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build(tmp_path_factory, "pool_plan", ["-O1"])


# (n, cached sizes in the order they were cached) -> (index of the block taken or -1, its size): literals worked from the rule
FIT = [
    ((4096, []), (-1, 0)),                                                     # an empty cache: the driver is asked
    ((4096, [4096]), (0, 4096)),                                               # an exact fit
    ((4096, [256, 3840]), (-1, 0)),                                            # nothing large enough
    ((4096, [4096 + 1024 + MIB]), (0, 4096 + 1024 + MIB)),                     # exactly n + n / 4 + 1 MiB: taken
    ((4096, [4096 + 1024 + MIB + 1]), (-1, 0)),                                # one byte over the slack: not taken
    ((4096, [4096 + 1024 + MIB + 1, 8192, 4352]), (2, 4352)),                  # the smallest block that is large enough, not the first
    ((4096, [2 * MIB, 3840]), (-1, 0)),                                        # the smallest large-enough block is over the slack: none (no look further down)
    ((4096, [8192, 8192, 8192]), (0, 8192)),                                   # several equal sizes: the one cached first
    ((8192, [4096, 8192, 8192, 12288]), (1, 8192)),
    ((1 << 30, [(1 << 30) + (1 << 28) + MIB, (1 << 30) + (1 << 28) + MIB + 256]), (0, (1 << 30) + (1 << 28) + MIB)),
    ((1 << 30, [(1 << 30) + (1 << 28) + MIB + 256]), (-1, 0)),
    ((256, [MIB + 320]), (0, MIB + 320)),                                      # 256 + 64 + 1 MiB
    ((256, [MIB + 321]), (-1, 0)),
    (((1 << 34) + 256, [(1 << 34) + 256]), (0, (1 << 34) + 256)),              # beyond 32 bits
]


@pytest.mark.parametrize("case,want", FIT)
def test_best_fit_takes_the_smallest_block_within_the_slack(plan, case, want):
    n, sizes = case
    fits = [(s, i) for i, s in enumerate(sizes) if s >= n]
    expect = (-1, 0)
    if fits:
        s, i = min(fits)                                                       # smallest size, then first cached
        if s <= n + n // 4 + MIB:
            expect = (i, s)
    assert expect == want, "the literal does not follow the stated rule"
    r = plan("fit", n, *sizes)
    assert (r["fit"], r["size"]) == want, r


@pytest.mark.parametrize("text,want", [("00", 0x00), ("ff", 0xFF), ("FF", 0xFF), ("55", 0x55), ("a5", 0xA5), ("fF", 0xFF), ("0a", 0x0A),
                                       ("", -1), ("5", -1), ("zz", -1), ("0x55", -1), ("555", -1), ("5 ", -1), (" 5", -1), ("5g", -1), ("-1", -1), ("+5", -1), ("f", -1)])
def test_the_knob_is_two_hex_digits_or_off(plan, text, want):
    assert plan("parse", text)["fill"] == want


def test_an_unset_knob_is_off(plan):
    assert plan("parse")["fill"] == -1


def test_requests_round_to_256_bytes_and_the_slack_of_a_filled_fresh_block_is_a_multiple_of_it(plan):
    for n, want in ((0, 256), (1, 256), (16, 256), (256, 256), (257, 512), (4095, 4096), ((1 << 32) + 1, (1 << 32) + 256)):
        r = plan("round", n)
        assert r["round"] == want
    assert r["slack"] > 0 and r["slack"] % 256 == 0


def test_the_header_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """A stand-alone host program with its own main, built with -fsanitize=address,undefined: any report makes it exit non-zero."""
    run = _build(tmp_path_factory, "pool_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for (n, sizes), want in FIT:
        r = run("fit", n, *sizes)
        assert (r["fit"], r["size"]) == want
    for text, want in (("00", 0), ("ff", 255), ("", -1), ("5", -1), ("zz", -1), ("0x55", -1)):
        assert run("parse", text)["fill"] == want
    assert run("parse")["fill"] == -1
