// compress.hip -- compress(x, q) of src/plotting.jl:38-47 on gfx950: clamp a matrix (optionally its log) to two of its own quantiles.
//
// The thresholds are Julia's default quantile (type 7) of all m values, which needs up to four order statistics (two neighbours per
// quantile).  They come from an exact radix select, not a sort: every value maps to an order-preserving 64-bit key (sign fold: -0.0 below
// +0.0, as isless), and the key of each wanted rank is fixed 8 bits at a time from the top.  A pass histograms that digit over the
// elements whose key still matches some wanted rank's prefix (at most four distinct prefixes, the `groups`): per-wave histograms in LDS
// with integer atomics, then one integer add per non-empty bin and workgroup to global memory.  Integer adds are exact, so the counts
// do not depend on arrival order.  Every pass also takes the AND and the OR of the keys of each group; a digit on which all keys of every
// group agree (AND and OR equal there) is read off the AND without a pass (`digits skipped`).  The matrix is re-read in every pass: no
// key array is kept.  With the fused log the select still runs on x itself: log is monotone, so the order statistics of log x are the
// logs of the order statistics of x, and only the (at most four) selected values go through the device's log -- the same function the
// last pass applies, element by element, before the clamp.  A NaN or a negative x (whose log is NaN) is flagged in the first pass.
#include "lpvs_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace lpvs {
namespace {

constexpr int kSelThreads = 256, kSelWaves = kSelThreads / 64;
constexpr int kMaxGroups = 4;
constexpr int64_t kSelPerThread = 16;                       // elements per thread and pass
constexpr int kStateWords = kMaxGroups * 256 + 2 * kMaxGroups + 1;   // histograms, ANDs, ORs, NaN flag (uint64 each)

thread_local double g_ctiming[5] = {0, 0, 0, 0, 0};

struct Groups {
    int ng = 1;
    unsigned long long prefix[kMaxGroups] = {0, 0, 0, 0};   // the key's bits above the digit of this pass
};

__host__ __device__ inline unsigned long long key_bits(double v) {
    unsigned long long b;
    memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double value_of_key(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}
// the value that is clamped: x or log(x), in the element's own precision, widened (exactly) to double
__device__ inline double value_of(double x, int take_log) { return take_log ? log(x) : x; }
__device__ inline double value_of(float x, int take_log) { return (double)(take_log ? logf(x) : x); }
// element e of the m = rows cols values sits at x[(e / rows) ld + e % rows]; 32-bit division when m allows it
__device__ inline int64_t offset_of(int64_t e, int64_t rows, int64_t ld, bool small) {
    if (small) {
        const uint32_t c = (uint32_t)e / (uint32_t)rows, r = (uint32_t)e - c * (uint32_t)rows;
        return (int64_t)c * ld + r;
    }
    const int64_t c = e / rows;
    return c * ld + (e - c * rows);
}

__device__ inline unsigned long long wave_and(unsigned long long v) {
    for (int o = 1; o < 64; o *= 2) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v &= ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ inline unsigned long long wave_or(unsigned long long v) {
    for (int o = 1; o < 64; o *= 2) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
        v |= ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// one digit pass: state = [group][256] counts of the digit at `shift` over the keys of x with (key >> (shift + 8)) == prefix[group], then
// the groups' ANDs, ORs of the whole keys and the NaN flag (take_log: also set by a negative x).
template <class T>
__global__ void __launch_bounds__(kSelThreads) select_hist_kernel(const T *x, int64_t rows, int64_t m, int64_t ld, int take_log, int shift, Groups G,
                                                                  unsigned long long *state) {
    __shared__ unsigned h[kSelWaves][kMaxGroups][256];
    __shared__ unsigned long long sand[kMaxGroups], sor[kMaxGroups];
    __shared__ int snan;
    const int tid = (int)threadIdx.x, w = tid / 64;
    for (int i = tid; i < kSelWaves * kMaxGroups * 256; i += kSelThreads) (&h[0][0][0])[i] = 0u;
    if (tid < kMaxGroups) { sand[tid] = ~0ull; sor[tid] = 0ull; }
    if (tid == 0) snan = 0;
    __syncthreads();
    unsigned long long a[kMaxGroups], o[kMaxGroups];
#pragma unroll
    for (int g = 0; g < kMaxGroups; ++g) { a[g] = ~0ull; o[g] = 0ull; }
    int nan = 0;
    const int top = shift + 8;
    const bool small = m < ((int64_t)1 << 31);
    constexpr int64_t kTile = (int64_t)kSelThreads * kSelPerThread;
    // the workgroups stride over the tiles: the per-workgroup flush to global (same few addresses for everyone) is paid once per workgroup
    for (int64_t e0 = (int64_t)blockIdx.x * kTile; e0 < m; e0 += (int64_t)gridDim.x * kTile) {
        T xv[kSelPerThread];
#pragma unroll
        for (int u = 0; u < kSelPerThread; ++u) {   // all loads of the tile in flight before the first is used
            const int64_t e = e0 + (int64_t)u * kSelThreads + tid;
            xv[u] = e < m ? x[offset_of(e, rows, ld, small)] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < kSelPerThread; ++u) {
            if (e0 + (int64_t)u * kSelThreads + tid >= m) continue;
            const double v = (double)xv[u];
            nan |= v != v || (take_log && v < 0.0);
            const unsigned long long key = key_bits(v), pre = top >= 64 ? 0ull : key >> top;
#pragma unroll
            for (int g = 0; g < kMaxGroups; ++g)
                if (g < G.ng && pre == G.prefix[g]) {
                    atomicAdd(&h[w][g][(unsigned)(key >> shift) & 255u], 1u);
                    a[g] &= key; o[g] |= key;
                }
        }
    }
#pragma unroll
    for (int g = 0; g < kMaxGroups; ++g) {
        if (g >= G.ng) break;
        const unsigned long long ra = wave_and(a[g]), ro = wave_or(o[g]);
        if ((tid & 63) == 0) { atomicAnd(&sand[g], ra); atomicOr(&sor[g], ro); }
    }
    if (nan) snan = 1;   // a plain store: the same value from every writer
    __syncthreads();
    for (int i = tid; i < G.ng * 256; i += kSelThreads) {
        const int g = i / 256, d = i - g * 256;
        unsigned long long sum = 0;
        for (int q = 0; q < kSelWaves; ++q) sum += h[q][g][d];
        if (sum) atomicAdd(&state[i], sum);
    }
    if (tid < G.ng) {
        atomicAnd(&state[kMaxGroups * 256 + tid], sand[tid]);
        atomicOr(&state[kMaxGroups * 256 + kMaxGroups + tid], sor[tid]);
    }
    if (tid == 0 && snan) atomicOr(&state[kMaxGroups * 256 + 2 * kMaxGroups], 1ull);
}

// out = clamp(v, lo, hi) (Julia's clamp: v > hi ? hi : v < lo ? lo : v), compared in double, stored in the element type
template <class T>
__global__ void __launch_bounds__(kSelThreads) clamp_kernel(const T *x, int64_t rows, int64_t m, int64_t ld, int take_log, double lo, double hi, T *out,
                                                            int64_t out_ld) {
    const int64_t e0 = (int64_t)blockIdx.x * (kSelThreads * kSelPerThread);
    const bool small = m < ((int64_t)1 << 31);
    for (int64_t u = 0; u < kSelPerThread; ++u) {
        const int64_t e = e0 + u * kSelThreads + threadIdx.x;
        if (e >= m) break;
        const double v = value_of(x[offset_of(e, rows, ld, small)], take_log);
        out[offset_of(e, rows, out_ld, small)] = (T)(v > hi ? hi : (v < lo ? lo : v));
    }
}
// the selected order statistics of x through the same log as the elements
template <class T> __global__ void log_values_kernel(double *v, int n) {
    if ((int)threadIdx.x < n) v[threadIdx.x] = value_of((T)v[threadIdx.x], 1);
}

// Julia's quantile (alpha = beta = 1) of m sorted values: the 0-based ranks of its two neighbours and the weight
struct Quant { int64_t j0 = 0, j1 = 0; double g = 0; };
Quant quantile_ranks(int64_t m, double p) {
    Quant q;
    if (m == 1) return q;
    const double aleph = (double)m * p + (1.0 - p);
    const int64_t j = std::min<int64_t>(std::max<int64_t>((int64_t)aleph, 1), m - 1);
    q.g = std::min(std::max(aleph - (double)j, 0.0), 1.0);
    q.j0 = j - 1; q.j1 = j;
    return q;
}
double interpolate(double a, double b, double g) {
    return (std::isfinite(a) && std::isfinite(b)) ? a + g * (b - a) : (1.0 - g) * a + g * b;
}

template <class T>
int32_t compress_impl(const T *x, int64_t rows, int64_t cols, int64_t ld, int32_t take_log, double qlo, double qhi, int32_t device, T *out, int64_t out_ld,
                      double *thresholds) {
    if (rows < 0 || cols < 0 || ld < rows || out_ld < rows) { set_error("need rows >= 0, cols >= 0, ld >= rows and out_ld >= rows (rows = %lld, cols = %lld, ld = %lld, out_ld = %lld)", (long long)rows, (long long)cols, (long long)ld, (long long)out_ld); return LPVS_EARGUMENT; }
    if (!(qlo >= 0.0 && qlo <= 1.0 && qhi >= 0.0 && qhi <= 1.0)) { set_error("quantile levels must lie in [0, 1] (got %g, %g)", qlo, qhi); return LPVS_EARGUMENT; }
    if (qlo > qhi) std::swap(qlo, qhi);
    const int64_t m = rows * cols;
    if (m == 0) { set_error("compress: the quantiles of an empty collection are undefined"); return LPVS_EDOMAIN; }
    if (!x || !out) { set_error("NULL argument"); return LPVS_EARGUMENT; }
    if (lpvs_device_count() == 0) { set_error("no HIP device visible (the gfx950 path has no CPU fallback)"); return LPVS_EDEVICE; }
    LPVS_HIP(hipSetDevice(device));
    StreamHolder sh;
    LPVS_HIP(hipStreamCreateWithFlags(&sh.s, hipStreamNonBlocking));
    const hipStream_t s = sh.s;
    Events<4> ev;
    for (auto &e : ev.e) LPVS_HIP(hipEventCreate(&e));
    DevBuf dx, dout, dstate;
    DrainOnExit drain(s);
    LPVS_HIP(hipEventRecord(ev.e[0], s));
    // the sub-matrix on this device: columns 0 .. cols-1 at stride ld, the last one only `rows` long
    const int64_t span = (cols - 1) * ld + rows;
    const T *xd = x;
    const int owner = device_of_ptr(x);
    if (owner != device) {
        LPVS_TRY(dx.alloc(sizeof(T) * (size_t)span));
        if (owner >= 0) LPVS_HIP(hipMemcpyPeerAsync(dx.p, device, x, owner, sizeof(T) * (size_t)span, s));
        else LPVS_TRY(copy_to_device(dx.p, x, sizeof(T) * (size_t)span, s));
        xd = dx.as<T>();
    }
    const bool dev_out = device_of_ptr(out) == device;
    T *od = out;
    int64_t od_ld = out_ld;
    if (!dev_out) { LPVS_TRY(dout.alloc(sizeof(T) * (size_t)m)); od = dout.as<T>(); od_ld = rows; }
    LPVS_TRY(dstate.alloc(sizeof(unsigned long long) * kStateWords));
    if (ceil_div(m, (int64_t)kSelThreads * kSelPerThread) > ((int64_t)1 << 31) - 1) { set_error("compress: %lld values are too many", (long long)m); return LPVS_EUNSUPPORTED; }
    const unsigned nblk = (unsigned)ceil_div(m, (int64_t)kSelThreads * kSelPerThread);   // clamp pass: a tile per workgroup
    int cus = 0;
    LPVS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const unsigned nsel = std::min<unsigned>(nblk, (unsigned)std::max(cus, 1) * 8u);       // select passes: resident workgroups striding over the tiles

    // ---- select: the keys of the wanted ranks, 8 bits a pass
    const Quant Q[2] = {quantile_ranks(m, qlo), quantile_ranks(m, qhi)};
    int64_t rank[4] = {Q[0].j0, Q[0].j1, Q[1].j0, Q[1].j1};   // rank within the rank's group
    int grp[4] = {0, 0, 0, 0};
    Groups G;
    unsigned long long st[kStateWords];
    int passes = 0, skipped = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = 0; i < kStateWords; ++i) st[i] = 0ull;
        for (int g = 0; g < kMaxGroups; ++g) st[kMaxGroups * 256 + g] = ~0ull;
        LPVS_TRY(copy_to_device(dstate.p, st, sizeof st, s));
        select_hist_kernel<T><<<nsel, kSelThreads, 0, s>>>(xd, rows, m, ld, take_log, shift, G, dstate.as<unsigned long long>());
        LPVS_HIP(hipGetLastError());
        LPVS_TRY(copy_from_device(st, dstate.p, sizeof st, s));
        LPVS_HIP(hipStreamSynchronize(s));
        ++passes;
        if (st[kMaxGroups * 256 + 2 * kMaxGroups]) {
            set_error(take_log ? "compress: the logarithm of the input holds NaN (a NaN or negative power): its quantiles are undefined"
                               : "compress: the input holds NaN: its quantiles are undefined");
            return LPVS_EDOMAIN;
        }
        // each rank moves into the bin that holds it; the distinct (group, bin) pairs are the next groups
        Groups N;
        N.ng = 0;
        int ngrp[4];
        for (int i = 0; i < 4; ++i) {
            const unsigned long long *hist = st + grp[i] * 256;
            int64_t below = 0;
            int d = 0;
            while (d < 255 && below + (int64_t)hist[d] <= rank[i]) { below += (int64_t)hist[d]; ++d; }
            rank[i] -= below;
            const unsigned long long pre = (G.prefix[grp[i]] << 8) | (unsigned long long)d;
            int g = 0;
            while (g < N.ng && N.prefix[g] != pre) ++g;
            if (g == N.ng) N.prefix[N.ng++] = pre;
            ngrp[i] = g;
        }
        // the keys of each group before this pass narrowed it, ANDed and ORed: digits on which they all agree need no pass
        unsigned long long agree = ~0ull;
        unsigned long long gand[kMaxGroups];
        for (int i = 0; i < 4; ++i) {
            const unsigned long long a = st[kMaxGroups * 256 + grp[i]], o = st[kMaxGroups * 256 + kMaxGroups + grp[i]];
            agree &= ~(a ^ o);
            gand[ngrp[i]] = a;
        }
        for (int i = 0; i < 4; ++i) grp[i] = ngrp[i];
        G = N;
        while (shift >= 8 && ((agree >> (shift - 8)) & 255ull) == 255ull) {
            shift -= 8;
            for (int g = 0; g < G.ng; ++g) G.prefix[g] = (G.prefix[g] << 8) | ((gand[g] >> shift) & 255ull);
            ++skipped;
        }
    }
    double v[4];
    for (int i = 0; i < 4; ++i) v[i] = value_of_key(G.prefix[grp[i]]);
    if (take_log) {
        LPVS_TRY(copy_to_device(dstate.p, v, sizeof v, s));
        log_values_kernel<T><<<1, 64, 0, s>>>(dstate.as<double>(), 4);
        LPVS_HIP(hipGetLastError());
        LPVS_TRY(copy_from_device(v, dstate.p, sizeof v, s));
        LPVS_HIP(hipStreamSynchronize(s));
    }
    const double t0 = m == 1 ? v[0] : interpolate(v[0], v[1], Q[0].g), t1 = m == 1 ? v[2] : interpolate(v[2], v[3], Q[1].g);
    LPVS_HIP(hipEventRecord(ev.e[1], s));
    clamp_kernel<T><<<nblk, kSelThreads, 0, s>>>(xd, rows, m, ld, take_log, t0, t1, od, od_ld);
    LPVS_HIP(hipGetLastError());
    LPVS_HIP(hipEventRecord(ev.e[2], s));
    if (!dev_out)
        LPVS_HIP(hipMemcpy2DAsync(out, sizeof(T) * (size_t)out_ld, od, sizeof(T) * (size_t)rows, sizeof(T) * (size_t)rows, (size_t)cols, hipMemcpyDefault, s));
    LPVS_HIP(hipEventRecord(ev.e[3], s));
    LPVS_HIP(hipStreamSynchronize(s));
    if (thresholds) { thresholds[0] = t0; thresholds[1] = t1; }
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) LPVS_HIP(hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]));
    g_ctiming[0] = passes; g_ctiming[1] = ms[0]; g_ctiming[2] = ms[1]; g_ctiming[3] = (double)ms[0] + ms[1] + ms[2]; g_ctiming[4] = skipped;
    return LPVS_OK;
}

}  // namespace
}  // namespace lpvs

using namespace lpvs;

extern "C" {

int32_t lpvs_compress_f64(const double *x, int64_t rows, int64_t cols, int64_t ld, int32_t take_log, double qlo, double qhi, int32_t device,
                          double *out, int64_t out_ld, double *thresholds) {
    try { return compress_impl(x, rows, cols, ld, take_log, qlo, qhi, device, out, out_ld, thresholds); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_compress_f32(const float *x, int64_t rows, int64_t cols, int64_t ld, int32_t take_log, double qlo, double qhi, int32_t device,
                          float *out, int64_t out_ld, double *thresholds) {
    try { return compress_impl(x, rows, cols, ld, take_log, qlo, qhi, device, out, out_ld, thresholds); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return LPVS_ENOMEM; }
}
int32_t lpvs_compress_last_timing(double *out, int32_t n) {
    return copy_timing(out, n, g_ctiming, 5);
}

}  // extern "C"
