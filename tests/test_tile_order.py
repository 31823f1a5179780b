"""The tile order of the one-launch ADMM iteration (csrc/tile_order.h): which tile workgroup bx of a launch takes, forward on even launches,
the tiles below the diagonal mirrored in groups of eight on odd ones.  The header has no HIP dependency: a tiny host program is built
against it and prints the map; CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "lpvspectral.jl_amd", "csrc")

PROGRAM = r"""
#include "tile_order.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    const int nblk = atoi(argv[1]), odd = atoi(argv[2]), n = nblk * (nblk + 1) / 2;
    for (int bx = 0; bx < n; ++bx) printf("%d\n", lpvs::tile_order_index(bx, nblk, odd));
    return 0;
}
"""


def _compiler():
    for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/bin/amdclang++", "/opt/rocm/bin/hipcc"):
        if os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def tile_order(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler under /opt/rocm")
    d = tmp_path_factory.mktemp("tile_order")
    src, exe = os.path.join(d, "tile_order_dump.cpp"), os.path.join(d, "tile_order_dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = [cxx, "-O1", "-std=c++17", "-I", HEADER_DIR, src, "-o", exe]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["-x", "c++"]                             # (host only: the header must not need the HIP runtime)
    subprocess.check_call(cmd)

    def run(nblk, odd):
        out = subprocess.check_output([exe, str(nblk), str(odd)], text=True)
        return [int(v) for v in out.split()]
    yield run
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("nblk", list(range(16, 65)) + [256])
def test_tile_order_is_an_xcd_preserving_involution(tile_order, nblk):
    n, T = nblk * (nblk + 1) // 2, nblk * (nblk - 1) // 2
    even, odd = tile_order(nblk, 0), tile_order(nblk, 1)
    assert len(even) == len(odd) == n
    assert even == list(range(n))                            # even parity is the order of every launch before the map existed
    for m in (even, odd):
        assert sorted(m) == list(range(n))                   # a bijection of [0, nblk (nblk + 1) / 2)
        assert m[:nblk] == list(range(nblk))                 # the diagonal tiles stay in front, each in its place
        assert all((m[bx] - nblk) % 8 == (bx - nblk) % 8 for bx in range(nblk, n))   # k mod 8 kept: the XCD under a round-robin deal
        assert all(m[m[bx]] == bx for bx in range(n))        # applied twice: the identity
    # what the odd map is for: the first workgroups below the diagonal take the last whole group of eight, and so on backwards
    Q = T // 8
    if Q > 0:
        assert odd[nblk:nblk + 8] == [nblk + 8 * (Q - 1) + r for r in range(8)]
        assert odd[nblk + 8 * (Q - 1):nblk + 8 * Q] == [nblk + r for r in range(8)]
    assert odd[nblk + 8 * Q:] == list(range(nblk + 8 * Q, n))   # the ragged T mod 8 tiles keep their place
