// pool_plan.h -- the two pure decisions of the caching device allocator (api.hip: DevBuf::alloc), without HIP: which cached block answers
// a request (best fit within a slack), and what the experiment knob LPVS_POOL_FILL asks for.  Host-testable: tests/test_pool_plan.py builds
// a stand-alone program against this header as it is.
#pragma once
#include <stddef.h>
#include <map>

namespace lpvs {

// A request is rounded up to a multiple of 256 bytes (at least one such unit) before anything else looks at it.
inline size_t pool_round(size_t nbytes) {
    if (nbytes == 0) nbytes = 16;
    return (nbytes + 255) & ~(size_t)255;
}

// The largest cached block a request of n bytes takes: n plus a quarter of it plus 1 MiB.
inline size_t pool_fit_limit(size_t n) { return n + n / 4 + ((size_t)1 << 20); }

// Best fit: the SMALLEST cached block of at least n bytes, if it is no larger than pool_fit_limit(n); end() otherwise (the caller asks
// the driver).  The cache is keyed by the blocks' true sizes; among blocks of one size the one cached first is taken.
template <class V>
inline typename std::multimap<size_t, V>::const_iterator pool_best_fit(const std::multimap<size_t, V> &cache, size_t n) {
    auto it = cache.lower_bound(n);
    return (it != cache.end() && it->first <= pool_fit_limit(n)) ? it : cache.end();
}

// LPVS_POOL_FILL (experiment knob): exactly two hexadecimal digits, either case -- the byte every block is filled with
// before DevBuf::alloc hands it out.  Anything else (null, empty, one digit, a prefix, a third character): -1, the knob is off.
inline int pool_fill_parse(const char *s) {
    if (s == nullptr) return -1;
    int v = 0;
    for (int i = 0; i < 2; ++i) {
        const char c = s[i];
        int d;
        if (c >= '0' && c <= '9') d = c - '0';
        else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
        else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
        else return -1;                                    // (the terminating NUL of a shorter string lands here too)
        v = v * 16 + d;
    }
    return s[2] == 0 ? v : -1;
}

// With the knob on, a FRESH block is asked for this much larger than the request, so its true size exceeds the request as a reused
// block's does (a multiple of 256 bytes; more than a tile row of doubles, so that a kernel that sizes itself by the block shows).
constexpr size_t kPoolFillSlack = 16 * 256;

}  // namespace lpvs
