// tile_order.h -- which tile a workgroup of the one-launch ADMM iteration takes ("tile order").  No HIP dependency: the
// host-side test (tests/test_tile_order.py) and tools/stream_read.hip compile it as it is.
#pragma once

#if defined(__HIPCC__)
#define LPVS_TILE_ORDER_HD __host__ __device__
#else
#define LPVS_TILE_ORDER_HD
#endif

namespace lpvs {

// Workgroup bx of a launch with nblk (nblk + 1) / 2 workgroups -> its place in the FORWARD order: the nblk diagonal tiles first, then
// the k-th tile below the diagonal at nblk + k (k = I (I - 1) / 2 + J, J < I).
//   even launches (odd == 0): the forward order itself.
//   odd launches: the tiles below the diagonal in groups of eight, the groups backwards -- k -> 8 (Q - 1 - k / 8) + k % 8 with
//   Q = T / 8 whole groups among the T = nblk (nblk - 1) / 2 tiles; the ragged T % 8 at the end keep their place.
// The first workgroups of a launch then ask for the tiles the last workgroups of the launch before it read, which are the lines that
// launch left in L2; k % 8 is kept, and with it the XCD under the round-robin deal of workgroups, so they ask the L2 that holds them.
// The diagonal tiles stay in front in both directions (the longest prologue, and at cfg3 the 96 KB float-head tiles: never the last
// workgroups of a launch).  The map is an involution, and any bijection gives the same bits: the tile sums are integer atomics.
LPVS_TILE_ORDER_HD inline int tile_order_index(int bx, int nblk, int odd) {
    if (!odd || bx < nblk) return bx;
    const int k = bx - nblk, Q = (nblk * (nblk - 1) / 2) / 8;
    if (k >= 8 * Q) return bx;
    return nblk + 8 * (Q - 1 - k / 8) + k % 8;
}

}  // namespace lpvs
